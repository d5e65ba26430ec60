"""rt_denoise_shards_temporal against rt_denoise_temporal_fetch at 1200 x 800 (profiles/temporal_shards_timing.txt): a record, no threshold.

One process on one MI355X, cover scene, two frames of the orbit (0.5 degrees apart), samples 1..4 each (features after the same four).
Context A renders a frame whole.  Context B renders both frames once as --world cyclic shards of single rows and copies every shard's
hdr, sq, feat and id strips device to device into its slot of the frame's parts buffers (0xff-filled: padding that is read would turn
the result into NaN).  Context C, which holds no scene, runs the sharded call.  A timed call always reads a history that is one frame
of orbit old: whole form -- render frame 0, call, upload and render frame 1, timed call; sharded form -- reset, call on frame 0's parts,
timed call on frame 1's.  Both fetches, the default parameters, --rounds rounds with the two forms interleaved, best of --best HIP-event
times per cell; the two must give the same den, den_var and history (sha256 printed).  The difference is the prepare pass reading the
current frame through the row mapping instead of straight down the strip; the history gather, the levels and the tonemap are the same.

usage: python tools/temporal_shards_timing.py [--world 8] [--rounds 3] [--best 5] > profiles/temporal_shards_timing.txt"""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--best", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from cpuraytracer_amd import HipRenderer, scenes, distributed as D
    W, H, n, world, deg = 1200, 800, 4, args.world, 0.5
    os.environ.pop("RT_DENOISE_STAGE", None)
    print("rt_denoise_shards_temporal (%d shards of single rows) against rt_denoise_temporal_fetch at %d x %d, cover scene, samples 1..%d per frame,"
          "\na history one frame of orbit (%.1f degrees) old; kernel sources %s" % (world, W, H, n, deg, bench.kernel_sources_hash()[:16]))
    frames = []
    for f in range(2):
        sc = scenes.build_scene("cover", bench.SCENE_SEED, W, H)
        sc.camera = scenes.orbit_camera(sc.camera, deg * f, (0.0, 1.0, 0.0))
        frames.append(sc)
    maps = open("/proc/self/maps").read()
    hiprt = C.CDLL(next(l.split()[-1] for l in maps.splitlines() if "libamdhip64.so" in l))
    rows_max = D.max_local_rows(H, world)
    px = rows_max * W
    parts = []
    b = HipRenderer(0)
    for f, sc in enumerate(frames):
        ptrs = []
        for c in (3, 3, 8, 1):
            p = C.c_void_p()
            if hiprt.hipMalloc(C.byref(p), C.c_size_t(world * px * c * 4)) != 0 or hiprt.hipMemset(p, C.c_int(0xff), C.c_size_t(world * px * c * 4)) != 0:
                raise SystemExit("hipMalloc / hipMemset failed")
            ptrs.append(p)
        hiprt.hipDeviceSynchronize()
        b.upload(sc)
        b.set_noise_estimate(True)
        for s in range(world):
            rs = D.shard_rowset(H, s, world)
            b.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED + f, rowset=rs, stats=False)
            b.render_features(W, H, 1, 1 + n, rowset=rs)
            b.copy_to_device(ptrs[0].value + s * px * 12, None)
            b.copy_moments_to_device(ptrs[1].value + s * px * 12)
            b.copy_features_to_device(ptrs[2].value + s * px * 32, ptrs[3].value + s * px * 4)
        b.synchronize()
        parts.append(ptrs)
    b.close()
    a, c = HipRenderer(0), HipRenderer(0)

    def digest(r):
        d, t = r.download_denoised(), r.download_temporal()
        return hashlib.sha256(b"".join(x.tobytes() for x in (d["rgb"], d["var"], t["state"], t["len"], t["target"]))).hexdigest()[:16]

    def render_whole(f):
        a.upload(frames[f])
        a.set_noise_estimate(True)
        a.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED + f, stats=False)
        a.render_features(W, H, 1, 1 + n)

    def whole(fetch, best):
        out = []
        for _ in range(best):
            a.temporal_reset()
            render_whole(0)
            a.denoise_temporal(fetch=fetch)
            render_whole(1)
            out.append(a.denoise_temporal(fetch=fetch, timed=True))
        return min(out)

    def sharded_call(f, fetch, timed):
        p = parts[f]
        return c.denoise_shards_temporal(p[0].value, p[1].value, p[2].value, p[3].value, W, H, world, rows_max, n, n, frames[f].camera, fetch=fetch, timed=timed)

    def sharded(fetch, best):
        out = []
        for _ in range(best):
            c.temporal_reset()
            sharded_call(0, fetch, False)
            out.append(sharded_call(1, fetch, True))
        return min(out)

    for fetch in (1, 4):  # warm-up: buffers, code objects
        whole(fetch, 1), sharded(fetch, 1)
    print("\nHIP-event time of the whole call (prepare pass with the history gather, 3 levels, tonemap), %d rounds interleaved, best of %d per cell, ms:"
          % (args.rounds, args.best))
    print("  fetch  round  rt_denoise_temporal_fetch  rt_denoise_shards_temporal  shards - whole  sha256 (whole)    same bits")
    T = {}
    for rnd in range(args.rounds):
        for fetch in (1, 4):
            t0 = whole(fetch, args.best)
            h0 = digest(a)
            t1 = sharded(fetch, args.best)
            h1 = digest(c)
            T.setdefault(fetch, []).append((t0, t1))
            print("  %5d  %5d  %25.4f  %26.4f  %+14.4f  %-16s  %s" % (fetch, rnd + 1, t0, t1, t1 - t0, h0, "yes" if h0 == h1 else "NO (%s)" % h1))
    print("\nbest over the rounds and run-to-run spread (largest - smallest of the rounds' bests), ms:")
    for fetch in (1, 4):
        w, s = [t[0] for t in T[fetch]], [t[1] for t in T[fetch]]
        print("  fetch %d: rt_denoise_temporal_fetch %.4f (spread %.4f)  rt_denoise_shards_temporal %.4f (spread %.4f)  difference %+.4f (%+.1f %%)"
              % (fetch, min(w), max(w) - min(w), min(s), max(s) - min(s), min(s) - min(w), 100.0 * (min(s) - min(w)) / min(w)))
    print("\nthe prepare pass reads %d pixels x 60 B of the current frame (hdr 12, sq 12, feat 32, id 4) either way; the parts form reads them row by"
          "\nrow from %d parts, after one integer divide and a table-free locate per pixel." % (W * H, world))
    for ptrs in parts:
        for p in ptrs:
            hiprt.hipFree(p)
    a.close()
    c.close()


if __name__ == "__main__":
    main()
