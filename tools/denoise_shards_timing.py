"""rt_denoise_shards against rt_denoise at 1200 x 800 (profiles/denoise_shards_timing.txt): a record, no threshold.

One process on one MI355X, cover scene, samples 1..4 (features after the same four).  Context A renders the whole image; context B
renders it again as --world cyclic shards of single rows and copies every shard's hdr, sq and feat strips device to device into its
slot of the parts buffers (0xff-filled: padding that is read would turn the result into NaN).  Then, on context A, for levels 1, 3, 5:
rt_denoise and rt_denoise_shards interleaved, --rounds rounds, best of --best HIP-event times each; the two must give the same den
and den_var (sha256 printed).  The difference is the prepare pass reading through the row mapping instead of straight down the strip;
the levels and the tonemap are the same launches.

usage: python tools/denoise_shards_timing.py [--world 8] [--rounds 3] [--best 5] > profiles/denoise_shards_timing.txt"""
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
    W, H, n, world = 1200, 800, 4, args.world
    os.environ.pop("RT_DENOISE_STAGE", None)
    print("rt_denoise_shards (%d shards of single rows) against rt_denoise at %d x %d, cover scene, samples 1..%d; kernel sources %s"
          % (world, W, H, n, bench.kernel_sources_hash()[:16]))
    sc = scenes.build_scene("cover", bench.SCENE_SEED, W, H)
    a = HipRenderer(0)
    a.upload(sc)
    a.set_noise_estimate(True)
    a.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED)
    a.render_features(W, H, 1, 1 + n)
    maps = open("/proc/self/maps").read()
    hiprt = C.CDLL(next(l.split()[-1] for l in maps.splitlines() if "libamdhip64.so" in l))
    rows_max = D.max_local_rows(H, world)
    px = rows_max * W
    ptrs = []
    for c in (3, 3, 8):
        p = C.c_void_p()
        if hiprt.hipMalloc(C.byref(p), C.c_size_t(world * px * c * 4)) != 0 or hiprt.hipMemset(p, C.c_int(0xff), C.c_size_t(world * px * c * 4)) != 0:
            raise SystemExit("hipMalloc / hipMemset failed")
        ptrs.append(p)
    hiprt.hipDeviceSynchronize()
    b = HipRenderer(0)
    b.upload(sc)
    b.set_noise_estimate(True)
    for s in range(world):
        rs = D.shard_rowset(H, s, world)
        b.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED, rowset=rs, stats=False)
        b.render_features(W, H, 1, 1 + n, rowset=rs)
        b.copy_to_device(ptrs[0].value + s * px * 12, None)
        b.copy_moments_to_device(ptrs[1].value + s * px * 12)
        b.copy_features_to_device(ptrs[2].value + s * px * 32, None)
    b.synchronize()
    b.close()

    def digest():
        d = a.download_denoised()
        return hashlib.sha256(d["rgb"].tobytes() + d["var"].tobytes()).hexdigest()[:16]

    def whole(levels, best):
        p = _capi.denoise_params(levels=levels)
        return min(a.denoise(p, timed=True) for _ in range(best))

    def parts(levels, best):
        p = _capi.denoise_params(levels=levels)
        return min(a.denoise_shards(ptrs[0].value, ptrs[1].value, ptrs[2].value, W, H, world, rows_max, n, n, params=p, timed=True) for _ in range(best))

    for L in (1, 3, 5):  # warm-up: buffers, code objects
        whole(L, 1), parts(L, 1)
    print("\nHIP-event time of the whole call (prepare pass, levels, tonemap), %d rounds interleaved, best of %d per cell, ms:" % (args.rounds, args.best))
    print("  levels  round  rt_denoise  rt_denoise_shards  shards - whole  den sha256 (whole)  same den")
    T = {}
    for rnd in range(args.rounds):
        for L in (1, 3, 5):
            t0 = whole(L, args.best)
            h0 = digest()
            t1 = parts(L, args.best)
            h1 = digest()
            T.setdefault(L, []).append((t0, t1))
            print("  %6d  %5d  %10.4f  %17.4f  %+14.4f  %-18s  %s" % (L, rnd + 1, t0, t1, t1 - t0, h0, "yes" if h0 == h1 else "NO (%s)" % h1))
    print("\nbest over the rounds, ms:")
    for L in (1, 3, 5):
        t0, t1 = min(t[0] for t in T[L]), min(t[1] for t in T[L])
        print("  levels %d: rt_denoise %.4f  rt_denoise_shards %.4f  difference %+.4f (%+.1f %%)" % (L, t0, t1, t1 - t0, 100.0 * (t1 - t0) / t0))
    print("\nthe prepare pass reads %d pixels x 56 B (hdr 12, sq 12, feat 32) and writes 48 B each, either way: %.1f MB; the parts form reads"
          "\nthe same bytes, row by row from %d parts." % (W * H, W * H * 104 / 1e6, world))
    for p in ptrs:
        hiprt.hipFree(p)
    a.close()


if __name__ == "__main__":
    main()
