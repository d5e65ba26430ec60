"""rt_denoise_shards_variance / rt_denoise_shards_temporal_variance against rt_denoise_variance / rt_denoise_temporal_variance at
1200 x 800 and ONE sample per pixel (profiles/denoise_shards_spatial_timing.txt): a record, no threshold.

One process on one MI355X, cover scene, two frames of the orbit (0.5 degrees apart), sample 1 each with the noise estimate off (features
after the same one sample).  Context A renders a frame whole.  Context B renders both frames once as --world cyclic shards of single rows
and copies every shard's hdr, feat and id strips device to device into its slot of the frame's parts buffers (0xff-filled: padding that
is read would turn the result into NaN); there is no buffer of second moments.  Context C, which holds no scene, runs the sharded calls.
Rows: radius 1..3 x {no history, nearest, bilinear}.  A timed temporal call always reads a history that is one frame of orbit old: whole
form -- render frame 0, call, upload and render frame 1, timed call; sharded form -- reset, call on frame 0's parts, timed call on frame
1's.  Default parameters, --rounds rounds with the two forms interleaved cell by cell, best of --best HIP-event times per cell after a
warm-up pass over every cell; the two forms must give the same den, den_var and history (sha256 printed).  The yardstick of a sharded
cell is the contiguous cell of this run plus this run's spread (largest - smallest of the rounds' bests of either form).

usage: python tools/denoise_shards_spatial_timing.py [--world 8] [--rounds 3] [--best 5] > profiles/denoise_shards_spatial_timing.txt"""
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
    from cpuraytracer_amd import HipRenderer, _capi, scenes, distributed as D
    W, H, n, world, deg = 1200, 800, 1, args.world, 0.5
    os.environ.pop("RT_DENOISE_STAGE", None)
    print("rt_denoise_shards_variance / rt_denoise_shards_temporal_variance (%d shards of single rows, RT_VARIANCE_SPATIAL) against"
          "\nrt_denoise_variance / rt_denoise_temporal_variance at %d x %d, cover scene, sample 1 per frame, the noise estimate off,"
          "\na history one frame of orbit (%.1f degrees) old; kernel sources %s" % (world, W, H, deg, bench.kernel_sources_hash()[:16]))
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
        for c in (3, 8, 1):
            p = C.c_void_p()
            if hiprt.hipMalloc(C.byref(p), C.c_size_t(world * px * c * 4)) != 0 or hiprt.hipMemset(p, C.c_int(0xff), C.c_size_t(world * px * c * 4)) != 0:
                raise SystemExit("hipMalloc / hipMemset failed")
            ptrs.append(p)
        hiprt.hipDeviceSynchronize()
        b.upload(sc)
        b.set_noise_estimate(False)
        for s in range(world):
            rs = D.shard_rowset(H, s, world)
            b.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED + f, rowset=rs, stats=False)
            b.render_features(W, H, 1, 1 + n, rowset=rs)
            b.copy_to_device(ptrs[0].value + s * px * 12, None)
            b.copy_features_to_device(ptrs[1].value + s * px * 32, ptrs[2].value + s * px * 4)
        b.synchronize()
        parts.append(ptrs)
    b.close()
    a, c = HipRenderer(0), HipRenderer(0)

    def digest(r, temporal):
        d = r.download_denoised()
        xs = [d["rgb"], d["var"]]
        if temporal:
            t = r.download_temporal()
            xs += [t["state"], t["len"], t["target"]]
        return hashlib.sha256(b"".join(x.tobytes() for x in xs)).hexdigest()[:16]

    def render_whole(f):
        a.upload(frames[f])
        a.set_noise_estimate(False)
        a.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED + f, stats=False)
        a.render_features(W, H, 1, 1 + n)

    def whole(V, fetch, best):
        out = []
        for _ in range(best):
            if fetch == 0:
                render_whole(1)
                out.append(a.denoise(variance=V, timed=True))
                continue
            a.temporal_reset()
            render_whole(0)
            a.denoise_temporal(fetch=fetch, variance=V)
            render_whole(1)
            out.append(a.denoise_temporal(fetch=fetch, variance=V, timed=True))
        return min(out)

    def sharded_call(V, f, fetch, timed):
        p = parts[f]
        if fetch == 0:
            return c.denoise_shards(p[0].value, None, p[1].value, W, H, world, rows_max, n, n, timed=timed, variance=V)
        return c.denoise_shards_temporal_variance(p[0].value, None, p[1].value, p[2].value, W, H, world, rows_max, n, n, frames[f].camera, fetch=fetch,
                                                  timed=timed, variance=V)

    def sharded(V, fetch, best):
        out = []
        for _ in range(best):
            if fetch != 0:
                c.temporal_reset()
                sharded_call(V, 0, fetch, False)
            out.append(sharded_call(V, 1, fetch, True))
        return min(out)

    cells = [(R, fetch) for R in (1, 2, 3) for fetch in (0, 1, 4)]
    Vs = {R: _capi.variance_params(source=_capi.RT_VARIANCE_SPATIAL, radius=R) for R in (1, 2, 3)}
    for R, fetch in cells:  # warm-up: buffers, code objects
        whole(Vs[R], fetch, 1), sharded(Vs[R], fetch, 1)
    print("\nHIP-event time of the whole call (spatial pass, prepare pass with the history gather where there is one, 3 levels, tonemap),"
          "\n%d rounds interleaved, best of %d per cell, ms (fetch 0: no history, rt_denoise_variance / rt_denoise_shards_variance):" % (args.rounds, args.best))
    print("  R  fetch  round  contiguous   shards  shards - contiguous  sha256 (contiguous)  same bits")
    T = {}
    for rnd in range(args.rounds):
        for R, fetch in cells:
            t0 = whole(Vs[R], fetch, args.best)
            h0 = digest(a, fetch != 0)
            t1 = sharded(Vs[R], fetch, args.best)
            h1 = digest(c, fetch != 0)
            T.setdefault((R, fetch), []).append((t0, t1))
            print("  %d  %5d  %5d  %10.4f  %7.4f  %+19.4f  %-19s  %s" % (R, fetch, rnd + 1, t0, t1, t1 - t0, h0, "yes" if h0 == h1 else "NO (%s)" % h1))
    print("\nbest over the rounds, this run's spread (largest - smallest of the rounds' bests, the larger of the two forms'), the yardstick"
          "\n(contiguous + spread) and the sharded cell against it, ms:")
    print("  R  fetch  contiguous  (spread)   shards  (spread)  difference      %   yardstick  within")
    over = 0
    for R, fetch in cells:
        w, s = [t[0] for t in T[(R, fetch)]], [t[1] for t in T[(R, fetch)]]
        spread = max(max(w) - min(w), max(s) - min(s))
        ok = min(s) <= min(w) + spread
        over += not ok
        print("  %d  %5d  %10.4f  (%.4f)  %7.4f  (%.4f)  %+10.4f  %+5.1f  %10.4f  %s" % (R, fetch, min(w), max(w) - min(w), min(s), max(s) - min(s), min(s) - min(w),
                                                                                     100.0 * (min(s) - min(w)) / min(w), min(w) + spread, "yes" if ok else "NO"))
    print("\n%d of %d sharded cells exceed their yardstick." % (over, len(cells)))
    print("\nthe spatial pass reads %d pixels x 44 B of the current frame (hdr 12, feat 32) either way, plus its halo; the parts form reads them row by"
          "\nrow from %d parts, after one locate per staged row of a tile.  The gather that feeds it carries 12 words per pixel (hdr 3, feat 8, id 1)"
          "\ninstead of 15: %d instead of %d bytes for this picture." % (W * H, world, W * H * 48, W * H * 60))
    for ptrs in parts:
        for p in ptrs:
            hiprt.hipFree(p)
    a.close()
    c.close()


if __name__ == "__main__":
    main()
