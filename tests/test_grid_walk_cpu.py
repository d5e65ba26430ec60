"""CPU emulation of the cell-grid scan's walk (rt_scan.h: grid_slab_rows + the feed of scan_list_grid), binary32 operation by
operation: the set of cells it visits for a segment must contain EVERY cell within D cells (Chebyshev) of the segment — that
is what makes the grid scan's candidate set conservative: the hit point of an accepted root lies on the clipped segment and
within r + reach of its sphere's centre, so the sphere's home cell is within D = (r_max + reach) / h of the segment.  No GPU."""
import ctypes as C

import numpy as np
import pytest

F = np.float32


def shipped_slab_rows(queries, ius, nv):
    """grid_segment_slope + grid_slab_rows AS SHIPPED: librt_hip.so's rt_unit_grid_rows runs the very functions of csrc/rt_scan.h
    (compiled for the host; no GPU needed), so an edit to them -- kGridSlack, the padding, the clamps -- meets these tests."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    L.rt_unit_grid_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 5)
    iu = np.ascontiguousarray(ius, dtype=np.int32)
    rows = np.zeros((q.shape[0], 2), dtype=np.int32)
    se = np.zeros(q.shape[0], dtype=np.float32)
    assert L.rt_unit_grid_rows(q.ctypes.data, iu.ctypes.data, q.shape[0], nv, rows.ctypes.data, se.ctypes.data) == 0
    return rows, se
SLACK = F(1e-3)


def fma(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def slab_rows(su, sv, eu, ev, D, iu, nv):
    """grid_slab_rows, same operations in the same order; returns (r0, r1) with r0 > r1 for 'no rows'"""
    du, dv = F(eu - su), F(ev - sv)
    ulo, uhi = min(su, eu), max(su, eu)
    a = max(ulo, F(F(F(iu) - D) - SLACK))
    b = min(uhi, F(F(F(iu + 1) + D) + SLACK))
    steep = abs(du) < F(F(1e-4) * max(abs(dv), F(1.0)))
    if steep:
        vlo, vhi = min(sv, ev), max(sv, ev)
    else:
        slope = F(dv / du)
        va, vb = fma(F(a - su), slope, sv), fma(F(b - su), slope, sv)
        pad = F(F(1e-4) * abs(slope))
        vlo, vhi = F(min(va, vb) - pad), F(max(va, vb) + pad)
    if a > b:
        return 1, 0
    f0 = np.floor(F(F(vlo - D) - SLACK))
    f1 = np.floor(F(F(vhi + D) + SLACK))
    r0 = 0 if f0 < 0 else int(f0)
    r1 = nv - 1 if f1 > nv - 1 else int(f1)
    if f1 < 0:
        r1 = -1
    return r0, r1


def walk(su, sv, eu, ev, D, nu, nv):
    """The slabs the feed of scan_list_grid lists, with the rows of each from the SHIPPED grid_slab_rows -- which must also equal
    the operation-by-operation model above (the model is the documentation; the shipped function is what is tested)."""
    fa = np.floor(F(F(min(su, eu) - D) - SLACK))
    fb = np.floor(F(F(max(su, eu) + D) + SLACK))
    iuA = 0 if fa < 0 else int(fa)
    iuB = nu - 1 if fb > nu - 1 else int(fb)
    cells = set()
    if iuA <= iuB and fb >= 0:
        ius = list(range(iuA, iuB + 1))
        rows, _ = shipped_slab_rows([[su, sv, eu, ev, D]] * len(ius), ius, nv)
        for iu, (r0, r1) in zip(ius, rows.tolist()):
            m0, m1 = slab_rows(su, sv, eu, ev, D, iu, nv)
            assert (r0 > r1 and m0 > m1) or (r0, r1) == (m0, m1), ("shipped grid_slab_rows differs from its model", su, sv, eu, ev, D, iu)
            for iv in range(r0, r1 + 1):
                cells.add((iu, iv))
    return cells


@pytest.mark.parametrize("seed", range(6))
def test_walk_visits_every_cell_within_d_of_the_segment(seed):
    rng = np.random.default_rng(500 + seed)
    nu, nv = 40, 57
    missed = 0
    for _ in range(400):
        kind = rng.integers(0, 5)
        s = rng.uniform(-3, [nu + 3, nv + 3])
        e = rng.uniform(-3, [nu + 3, nv + 3])
        if kind == 1:    # nearly parallel to v
            e[0] = s[0] + rng.normal() * 10.0 ** rng.uniform(-9, -2)
        elif kind == 2:  # nearly parallel to u
            e[1] = s[1] + rng.normal() * 10.0 ** rng.uniform(-9, -2)
        elif kind == 3:  # short
            e = s + rng.normal(size=2) * 10.0 ** rng.uniform(-6, 0)
        elif kind == 4:  # ends on cell borders
            s, e = np.round(s), np.round(e * 2) / 2
        su, sv, eu, ev = F(s[0]), F(s[1]), F(e[0]), F(e[1])
        D = F(rng.choice([0.05, 0.4, 0.9, 1.6, 3.2]) * rng.uniform(0.5, 1.0))
        got = walk(su, sv, eu, ev, D, nu, nv)
        # every cell that holds a point within D (Chebyshev) of a point of the segment -- sampled densely, in binary64
        t = np.linspace(0.0, 1.0, 801)[:, None]
        pts = np.array([su, sv], dtype=np.float64) + t * (np.array([eu, ev], dtype=np.float64) - np.array([su, sv], dtype=np.float64))
        offs = np.float64(D) * (1.0 - 1e-6) * np.array([[-1, -1], [-1, 1], [1, -1], [1, 1], [0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]], dtype=np.float64)
        q = (pts[:, None, :] + offs[None, :, :]).reshape(-1, 2)
        c = np.floor(q).astype(np.int64)
        ok = (c[:, 0] >= 0) & (c[:, 0] < nu) & (c[:, 1] >= 0) & (c[:, 1] < nv)
        need = set(map(tuple, np.unique(c[ok], axis=0).tolist()))
        missed += len(need - got)
        # and the walk is not wildly generous: within D + 1.5 cells of the segment's bounding box
        for (iu, iv) in got:
            assert min(su, eu) - D - 1.5 <= iu + 1 and iu <= max(su, eu) + D + 1.5
    assert missed == 0


def _mixed_sign_layer(oracle, n=2400, side=20.0, seed=77):
    """A thin layer of small spheres over a floor, laid out for the cell grid.  Every third radius is negative and LARGER in size
    (|r| in 0.15 .. 0.2) than any positive one (0.05 .. 0.1): a dilation, a cell size or a clip box taken from the signed radii would
    be too small by a factor of two."""
    rng = np.random.default_rng(seed)
    centers = np.stack([rng.uniform(-side, side, n), 0.2 + rng.uniform(0, 0.05, n), rng.uniform(-side, side, n)], 1)
    radii = rng.uniform(0.05, 0.1, n)
    radii[::3] = -rng.uniform(0.15, 0.2, len(radii[::3]))
    sph = np.zeros(n + 1, dtype=oracle.SPHERE_DTYPE)
    sph["cx"][:n], sph["cy"][:n], sph["cz"][:n], sph["r"][:n] = centers[:, 0], centers[:, 1], centers[:, 2], radii
    sph[n] = (0.0, -1000.0, 0.0, 1000.0)
    return sph


def test_walk_visits_the_home_cell_of_every_sphere_the_oracle_accepts_on_a_mixed_sign_layer(built, oracle):
    """The property above on a real grid: rt_unit_grid_info gives the grid rt_scene_upload builds (origin, cell size, dilation
    D0 = max|r| / h, clip box, each sphere's home cell as the scan's cell table holds it).  Rays graze chosen spheres; for every ray
    whose root the oracle's Sphere::Intersect accepts (a one-sphere scene), the ray is clipped to the box in binary64, put into cell
    units as the kernel does, and walked with D0 alone (the kernel's D adds its rounding reach and slack: a smaller D asks more of
    the walk): the sphere's home cell must be among the cells visited.  Needs |r| in D0, in the cell size and in the box."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    sph = _mixed_sign_layer(oracle)
    n = len(sph)
    ou, of, home = (C.c_uint32 * 5)(), (C.c_float * 10)(), np.zeros(n, dtype=np.int32)
    _capi.check(L.rt_unit_grid_info(sph.ctypes.data, n, ou, of, home.ctypes.data))
    assert ou[0] == 1, "the layer scene must select the cell grid"
    nu, nv, axU, axV = int(ou[1]), int(ou[2]), int(ou[3]), int(ou[4])
    g0 = np.array([of[0], of[1]], dtype=np.float64)
    invH, D0 = np.float64(of[2]), F(of[3])
    lo, hi = np.array(of[4:7], dtype=np.float64), np.array(of[7:10], dtype=np.float64)
    small = np.nonzero(home >= 0)[0]
    assert len(small) == n - 1 and home[n - 1] == -1  # the floor is the one big sphere
    c = np.stack([sph["cx"], sph["cy"], sph["cz"]], 1).astype(np.float64)
    r = np.abs(sph["r"].astype(np.float64))
    # the tables enclose |r|: dilation, box, and every small sphere sits in the cell that holds its centre
    assert np.float64(D0) >= r[small].max() * invH and 1.0 / invH >= 2.5 * r[small].max()
    assert (c[small] - r[small, None] >= lo).all() and (c[small] + r[small, None] <= hi).all()
    cell = np.floor((c[small][:, [axU, axV]] - g0) * invH).astype(np.int64)
    assert (cell[:, 0] * nv + cell[:, 1] == home[small]).all()

    rng = np.random.default_rng(78)
    neg, pos = small[sph["r"][small] < 0], small[sph["r"][small] > 0]
    targets = np.concatenate([rng.choice(neg, 80, replace=False), rng.choice(pos, 40, replace=False)])
    ref = oracle.build_scene("three", 1, 1.5)
    one = oracle.Oracle()
    checked = checked_neg = far = 0
    for k in targets:
        rays = []
        for q in range(6):
            ang, dist = rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 15.0)
            height = [rng.uniform(0.5, 5.0), rng.uniform(0.5, 5.0), 0.225 + rng.normal() * 0.02, rng.uniform(-0.3, 0.15)][q % 4]  # above, level with the layer, below
            o = c[k] + np.array([dist * np.cos(ang), 0.0, dist * np.sin(ang)])
            o[1] = height
            to = c[k] - o
            perp = np.cross(to, rng.normal(size=3))
            perp /= np.linalg.norm(perp)
            aim = c[k] + perp * r[k] * rng.choice([0.2, 0.9, 0.99, 0.9999])  # grazing: the hit point is almost |r| from the centre
            d = (aim - o) / np.linalg.norm(aim - o) * rng.choice([1.0, 0.01, 30.0])
            rays.append(np.concatenate([o, d]))
        rays = np.array(rays, dtype=np.float32)
        mat = np.zeros(1, dtype=oracle.MATERIAL_DTYPE)
        one.upload(oracle.Scene(sph[k:k + 1], mat, ref.camera, ref.sun, ref.sky, ref.exposure_scale))
        hits = one.closest_hit(rays)
        for ray, hit in zip(rays.astype(np.float64), hits):
            if hit[1:2].view(np.int32)[0] < 0:
                continue
            o, d, t = ray[:3], ray[3:], np.float64(hit[0])
            with np.errstate(divide="ignore"):
                t0, t1 = (lo - o) / d, (hi - o) / d
            tn, tf = max(np.minimum(t0, t1).max(), 0.0), np.maximum(t0, t1).min()
            assert tn * (1 - 1e-5) - 1e-5 <= t <= tf * (1 + 1e-5) + 1e-5, ("the accepted hit lies outside the clip box", int(k), t, tn, tf)
            s, e = ((o + tn * d)[[axU, axV]] - g0) * invH, ((o + tf * d)[[axU, axV]] - g0) * invH
            got = walk(F(s[0]), F(s[1]), F(e[0]), F(e[1]), D0, nu, nv)
            assert (int(home[k]) // nv, int(home[k]) % nv) in got, ("the walk misses an accepted sphere's home cell", int(k), float(sph["r"][k]))
            checked += 1
            checked_neg += sph["r"][k] < 0
            far += np.abs((o + t * d) - c[k])[[axU, axV]].max() > 0.1  # farther from the centre than any positive radius
    one.close()
    # not vacuous: most rays are accepted, most of those on negative spheres, many of them beyond the reach of a signed maximum
    assert checked >= 400 and checked_neg >= 250 and far >= 100, (checked, checked_neg, far)
