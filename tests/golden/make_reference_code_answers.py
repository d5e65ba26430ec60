"""Writes tests/golden/reference_code_answers.npz: inputs, and the outputs that the reference's own compiled sources
(oracle/_ref/libref.so, see oracle/Makefile and oracle/ref_api.h) gave for them, for a fixed subset of what
tests/test_reference_code_cpu.py compares live -- so that the oracle stays pinned to the reference's code on machines where the
reference does not exist.  Where the libm rule applies (HaltonSampleDisk / Hemisphere, the diffuse bounce, Camera's tan) the
values the reference's libm returned are recorded beside their arguments.  Recorded data only; run from the repository root on
a machine that has the reference:  python tests/golden/make_reference_code_answers.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle_py as O  # noqa: E402
from oracle import ref_py as R  # noqa: E402
import test_reference_code_cpu as T  # noqa: E402  (input generators only)

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


def main():
    rng = np.random.default_rng(20260101)
    out = {}
    # (a)
    idx = np.unique(np.concatenate([np.arange(0, 600), rng.integers(0, 10**6, 1600)])).astype(np.uint64)
    out["halton_index"] = idx
    for base in (2, 3, 4, 5, 7):
        out["halton_%d" % base] = R.halton(idx, base)
    big = np.array([2**32 + k for k in range(-8, 9)] + [2**40, 2**63, 2**64 - 1], dtype=np.uint64)
    out["halton_big_index"], out["halton_big_3"] = big, R.halton(big, 3)
    midx = np.unique(np.concatenate([np.arange(0, 800), rng.integers(0, 300000, 1400)])).astype(np.uint64)
    out["map_index"] = midx
    out["disk"], out["hemisphere"] = R.halton_disk(midx, 4, 5), R.halton_hemisphere(midx, 5, 7)
    theta, phi = T.TWO_PI * R.halton(midx, 4), T.TWO_PI * R.halton(midx, 7)
    out["disk_cos_arg"] = out["disk_sin_arg"] = theta
    out["hem_cos_arg"] = out["hem_sin_arg"] = phi
    out["disk_cos"], out["disk_sin"] = R.libm(R.COS, theta), R.libm(R.SIN, theta)
    out["hem_cos"], out["hem_sin"] = R.libm(R.COS, phi), R.libm(R.SIN, phi)
    # (b)
    spheres = np.array([(0, 0, 0, 1), (0, -1000, 0, 1000), (0.3, 0.2, -7.1, 0.2), (1e6, -1e6, 1e6, 1e-3), (-31.5, 770.25, 12.0, 412.0),
                        (0.5, 0.25, 2, 0.0), (0.5, 0.25, 2, -0.75), (0, 0, 0.001 + 2.0 ** -10, 2.0 ** -10)], F)
    rays = []
    for k, s in enumerate(spheres):
        r = T.rays_for_sphere(rng, s[:3], s[3], 250)
        if k == 7:
            nb, _ = T.near_bound_rays(s[:3], s[3])
            r[:len(nb[:150])] = nb[:150]
        rays.append(r)
    out["sphere"], out["sphere_rays"] = spheres, np.array(rays)
    out["sphere_hits"] = np.array([R.sphere_intersect(s, r) for s, r in zip(spheres, rays)])
    # (d)
    focal = float(np.sqrt(T.dot3(np.array([12, 1, -2.5], F), np.array([12, 1, -2.5], F))))
    params = [(0, 0, 0, 0, 0, 1, 90.0, 2.0, 1.0, 0.0), (12, 2, -2.5, 0, 1, 0, 25.0, 1.5, focal, 0.4), (12, 2, -2.5, 0, 1, 0, 25.0, 1920 / 1080.0, focal, 2.0)]
    for _ in range(21):
        o = rng.normal(size=3) * 10 ** rng.uniform(-1, 2)
        params.append(tuple(o) + tuple(o + rng.normal(size=3) * 3) + (rng.uniform(1, 170), rng.uniform(0.3, 3), 10 ** rng.uniform(-1, 2), rng.uniform(0, 3)))
    params = np.array(params, F)
    out["camera_params"] = params
    cams = [R.camera_make(p[0:3], p[3:6], float(p[6]), float(p[7]), float(p[8]), float(p[9])) for p in params]
    out["camera_members"] = np.array([T.camera_members(c) for c in cams])
    out["camera_tan_arg"] = (params[:, 6] * F(3.141592654) / F(180.0)) / F(2.0)
    out["camera_tan"] = R.libm(R.TAN, out["camera_tan_arg"])
    q = np.concatenate([rng.uniform(-0.2, 1.2, (len(params), 60, 2)), rng.uniform(-1, 1, (len(params), 60, 2))], 2).astype(F)
    out["camera_uv_offset"] = q
    out["camera_rays"] = np.array([R.camera_ray(c, qq) for c, qq in zip(cams, q)])
    # (e)
    mats = [T.material_record(O, T.OPAQUE, 0, 16.0, rgb0=(0.4, 0.2, 0.1)), T.material_record(O, T.OPAQUE, 1, 0.0, tiling=10.0, rgb0=(0.9, 0.9, 0.9), rgb1=(0.2, 0.3, 0.1)),
            T.material_record(O, T.OPAQUE, 0, 37.5, rgb0=(0.123, 0.456, 0.789)), T.material_record(O, T.METAL, 0, 0.0, rgb0=(0.7, 0.6, 0.5)),
            T.material_record(O, T.METAL, 1, 1.0, tiling=4.0, rgb0=(0.05, 0.5, 0.95), rgb1=(1, 1, 1)), T.material_record(O, T.GLASS, 0, 16.0, ior=1.5),
            T.material_record(O, T.GLASS, 0, 1.0, ior=2.4), T.material_record(O, T.GLASS, 0, 8.0, ior=0.7), T.material_record(O, T.GLASS, 0, 8.0, ior=1.0),
            T.material_record(O, T.EMISSIVE, 1, 0.0, tiling=2.0, rgb0=(0.85, 0.91, 0.98), rgb1=(0.1, 0.1, 0.1), luminance=8000.0)]
    n = 200
    shade_spheres = np.array([(0, 0, 0, 1), (0, 3, 0, 1), (2.5, 2.5, 2.5, 0.8), (-3, 0.5, 1, 1.5)], F)
    uv = np.stack(np.meshgrid(np.linspace(-0.25, 1.25, 21), np.linspace(-0.25, 1.25, 21)), -1).reshape(-1, 2).astype(F)
    rs = R.Scene(T.flat_scene(O, shade_spheres).spheres)
    keys = ("scatter_in", "scatter_out", "scatter_counters", "scatter_hemisphere", "scatter_cos", "scatter_sin", "shade_lights", "shade_n_lights",
            "shade_view_origin", "shade_hits", "shade_out", "texture_out")
    acc = {k: [] for k in keys}
    for k, m in enumerate(mats):
        h = T.hits_for(rng, n, float(m["ior"][0]))
        mat = R.Material(m)
        r_out, cnt = mat.scatter(h)
        acc["scatter_in"].append(h), acc["scatter_out"].append(r_out), acc["scatter_counters"].append(cnt)
        acc["scatter_hemisphere"].append(R.halton_hemisphere(cnt[:, 0], 5, 7))
        phi = T.TWO_PI * R.halton(cnt[:, 0], 7)
        acc["scatter_cos"].append(R.libm(R.COS, phi)), acc["scatter_sin"].append(R.libm(R.SIN, phi))
        n_lights = (1, 0, 2, 3, 8)[k % 5]
        lights = T.shade_lights(O, rng, n_lights)
        rec = np.zeros((8, 7), F)
        for q, l in enumerate(lights):
            rec[q] = np.frombuffer(bytes(l), dtype=F)
        hits, vo = T.surface_hits(rng, n), (rng.normal(size=3) * 10).astype(F)
        shade, _ = mat.shade(hits, lights, vo, rs)
        acc["shade_lights"].append(rec), acc["shade_n_lights"].append(n_lights), acc["shade_view_origin"].append(vo)
        acc["shade_hits"].append(hits), acc["shade_out"].append(mat.emit(hits) + shade)
        acc["texture_out"].append(R.texture_eval(m, uv))
        mat.close()
    for k in keys:
        out[k] = np.array(acc[k])
    out["material"] = np.array([np.frombuffer(m.tobytes(), dtype=np.uint8) for m in mats])
    out["shade_spheres"], out["texture_uv"] = shade_spheres, uv
    path = os.path.join(HERE, "reference_code_answers.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
