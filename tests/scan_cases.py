"""Scenes and DIRECTED rays for the closest-hit scans (csrc/rt_scan.h), shared by tests/test_scan_rays_cpu.py (the generator's honesty,
on the oracle alone) and tests/test_scan_rays.py (the device).  numpy, the oracle and the GPU-less layout queries of the device
library; nothing here needs a GPU.

`scene_cases()` lists twelve small seeded scenes, each with the knobs and the scan variant it is meant for; `scene(oracle, name)`
builds one, `rays(oracle, name)` its rays: labelled classes, each built in binary64 and rounded to binary32 once.

  grazers    the ray's line passes the centre of a sampled sphere at |r| (1 + delta), delta = +-10^k, k uniform in [-8, -1.5]; origins
             0.5 to 4 |r| before the closest approach, or 10, 300, 3,000 scene extents before it; |d| = 1, 0.3, 5
  starters   what a bounce produces: the origin is the binary32 rounding of a surface point, moved 0, +-1, +-4 ulp along the normal; the
             direction a tangent +-[1e-6, 1e-2] inward or outward; and inward chords whose SECOND root is placed at the reference's
             bias 0.001: on it, +-1, +-8 ulp and +-1e-3 relative (spheres of radius 5e-4 .. 4e-3; some have a diameter below the bias)
  behind     rays all but tangent to a group bound of rt_unit_layout (centre C, radius Rf; normalised d.(o - C) = +-[1e-6, 1e-2]): half
             start on the shell (1 + delta) Rf, delta = +-[1e-7, 1e-2]; the bound carries the filter's margin, its members end mu Rf
             short of it, and none of these can hit the group.  The other half hit the cap of the member that reaches farthest
             out, a root just beyond the bias ahead, from e = [1e-7, 1e-2] of the members' reach below it (see _behind)
  near       two spheres on one ray with roots t and t (1 + eps), |eps| = 2^-9 .. 2^-24, either sign: a sphere B set into the top of a
             sphere A along a direction w -- a fifth of A's radius and standing 2^-9 R out of it, or 2.5 times A and more and 2^-9 R
             short of A's top -- and rays down w at the distance from the axis where the two surfaces are eps t apart; B comes before
             A in the list for half the pairs and after it for the other half
  ties       (three scenes) exact duplicates of a sphere at a distant list index, and mirror pairs about the plane z = z0 with the
             rays kept in that plane (o.z = z0, d.z = 0 exactly): o.z - c.z is +-the same value, so both roots have the same bits
  degenerate direction components exactly +0, -0, +-1e-30 and a denormal beside one component of +-1, 0.3, 5 along each axis; origins
             inside the scene's box, outside it, and within 4 ulp of the box's faces and (cell-grid scenes) of cell borders
  crowded    blocks of 64 consecutive rays that skim a row of spheres (the layer, for the cell-grid scenes), crossing dozens of group
             bounds each; then a whole wave that misses everything; then a wave of misses with ONE crowded ray in it
"""
import ctypes as C
import functools

import numpy as np

from test_primary_tables_fuzz import _scene
from test_shadow_index_cpu import environment

F = np.float32
BIAS = F(0.001)  # ray-tracing.cpp:52, as the comparison sees it
EPS_K = tuple(range(9, 25))  # |eps| = 2^-k of the near-equal roots
GRAZE_K = (-8.0, -1.5)
FAR = (10.0, 300.0, 3000.0)  # scene extents between a far origin and the closest approach
LENGTHS = (1.0, 0.3, 5.0)


class ScanCase:
    """name; spec of the scene (see _make); env: the knobs; variant: (kLds, kScan) of rt_trace_variants.h's RT_SCAN_VARIANTS the unit
    kernel must run; kind: what rt_unit_layout_info must say (0 flat, 1 cell grid, 2 hierarchy); image: also rendered."""

    def __init__(self, name, spec, env, variant, kind, image=False):
        self.name, self.spec, self.env, self.variant, self.kind, self.image = name, spec, env, variant, kind, image


def _spec(layout, n, seed, extent, negative=False, scale=1.0, offset=(0.0, 0.0, 0.0), ties=False):
    return dict(layout=layout, n=n, seed=seed, extent=extent, negative=negative, scale=scale, offset=offset, ties=ties)


_FLAT509 = _spec("box", 509, 3104, 8.0, ties=True)
_CASES = (
    ScanCase("flat5", _spec("box", 5, 3101, 8.0), {}, (True, 1), 0),
    ScanCase("flat37_negative_scale_1e-3", _spec("box", 37, 3102, 8.0, negative=True, scale=1e-3), {}, (True, 1), 0),
    ScanCase("flat64_offset_2e4", _spec("box", 64, 3103, 8.0, offset=(2e4, -1e4, 1.5e4)), {}, (True, 1), 0),
    ScanCase("flat509_ties", _FLAT509, {}, (True, 1), 0, image=True),
    ScanCase("flat512_negative_scale_1e3", _spec("box", 512, 3105, 8.0, negative=True, scale=1e3), {}, (True, 1), 0),
    ScanCase("hierarchy513", _spec("box", 513, 3106, 8.0), {}, (False, 2), 2),
    ScanCase("hierarchy1500_floor_ties", _spec("soup", 1500, 3107, 24.0, ties=True), {}, (False, 2), 2, image=True),
    ScanCase("hierarchy400_tree_top_16", _spec("soup", 400, 3108, 10.0), {"RT_TREE_TOP": "16"}, (False, 2), 2),
    ScanCase("hierarchy700_tree_lds_0", _spec("soup", 700, 3109, 16.0, negative=True), {"RT_TREE_LDS": "0"}, (False, 2), 2),
    ScanCase("grid3000_ties", _spec("layer", 3000, 3110, 30.0, negative=True, ties=True), {}, (False, 3), 1, image=True),
    ScanCase("valu509", _FLAT509, {"RT_SCAN": "valu"}, (True, 0), 0),
    ScanCase("valu509_global_tables", _FLAT509, {"RT_SCAN": "valu", "RT_FORCE_GLOBAL_TABLES": "1"}, (False, 0), 0),
)


def scene_cases():
    return _CASES


def case(name):
    return next(c for c in _CASES if c.name == name)


def scene_names():
    """The cases whose scene is their own: the two RT_SCAN=valu cases run flat509's scene and rays."""
    return [c.name for c in _CASES if not c.name.startswith("valu")]


# ------------------------------------------------------------------------------------------------ the device library's host queries
def layout(spheres):
    """rt_unit_layout under the environment of the moment: (orig [groups, 4], 0xffffffff = padding; bounds [groups, 4] = C, |C|^2 - Rf^2)."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    n = C.c_uint32(0)
    sph = np.ascontiguousarray(spheres)
    _capi.check(L.rt_unit_layout(sph.ctypes.data, sph.shape[0], 0, C.byref(n), None, None))
    orig = np.zeros(n.value * 4, dtype=np.uint32)
    bounds = np.zeros((n.value, 4), dtype=F)
    _capi.check(L.rt_unit_layout(sph.ctypes.data, sph.shape[0], n.value, C.byref(n), orig.ctypes.data, bounds.ctypes.data))
    return orig.reshape(-1, 4), bounds


def layout_info(spheres):
    from cpuraytracer_amd import _capi
    sph = np.ascontiguousarray(spheres)
    out = (C.c_uint32 * 5)()
    _capi.check(_capi.load().rt_unit_layout_info(sph.ctypes.data, sph.shape[0], out))
    return list(out)


def grid_info(spheres):
    """rt_unit_grid_info: None unless the scene selects the cell grid; else (nu, nv, axis u, axis v, origin u, origin v, 1 / cell
    size, home cell of every sphere)."""
    from cpuraytracer_amd import _capi
    sph = np.ascontiguousarray(spheres)
    ou, of, home = (C.c_uint32 * 5)(), (C.c_float * 10)(), np.zeros(len(sph), dtype=np.int32)
    _capi.check(_capi.load().rt_unit_grid_info(sph.ctypes.data, len(sph), ou, of, home.ctypes.data))
    if ou[0] != 1:
        return None
    return int(ou[1]), int(ou[2]), int(ou[3]), int(ou[4]), float(of[0]), float(of[1]), float(of[2]), home


def planned_scan(sc, env):
    """Word [26] of rt_unit_launch_plan (include/rt_api.h) for the scene under the knobs env, which must be those of the moment: what
    host/rt_launch_plan.cpp's PlanScanOnly -- the plan of rt_unit_closest_hit's own launch -- decides, as ((kLds, kScan), tree_in_lds,
    instantiated).  The case is filled from the layout queries: scan entries 4 x groups, levels, grid cells; the top level of the
    hierarchy as the builder makes it (groups, then every four nodes one, until at most RT_TREE_TOP are left); one light, the
    context's defaults (256 CUs; one block of 1024 threads per CU, or four of 256 under RT_SCAN=valu) and the knobs the cases set."""
    from cpuraytracer_amd import _capi
    info = layout_info(sc.spheres)
    orig, _ = layout(sc.spheres)
    top_max = int(env.get("RT_TREE_TOP", "128"))
    nodes, off, levels = len(orig), 0, 1
    while levels < info[4]:
        off, nodes, levels = off + nodes, (nodes + 3) // 4, levels + 1
    assert info[4] == 1 or nodes <= top_max
    mfma = env.get("RT_SCAN") != "valu"
    case_words = np.zeros(28, dtype=np.uint32)
    case_words[0:4] = (4 * len(orig), info[4], nodes, off)
    case_words[4] = 1 if info[0] == 1 else 0
    case_words[5:7] = (info[1], info[2])
    case_words[11:15] = (1, 256, 1 if mfma else 4, 1024 if mfma else 256)
    case_words[15] = (1 if mfma else 0) | 2 | 4 | 8 | (16 if env.get("RT_TREE_LDS", "1") != "0" else 0) | (32 if env.get("RT_FORCE_GLOBAL_TABLES", "0") != "0" else 0)
    case_words[24:26] = (64 * 1024, 6)
    plan = np.zeros(28, dtype=np.uint32)
    _capi.check(_capi.load().rt_unit_launch_plan(case_words.ctypes.data, 1, plan.ctypes.data))
    w = int(plan[26])
    return (bool(w & 1), (w >> 1) & 3), bool(w & 8), bool(w & 16)


def group_bounds(sc):
    """(group of every sphere, C [groups, 3], Rf [groups]) in binary64.  Rf from the stored |C|^2 - Rf^2 where that difference is well
    conditioned, else from the members (a scene far from the origin)."""
    orig, bounds = layout(sc.spheres)
    c, r = centres(sc), radii(sc)
    Cg = bounds[:, :3].astype(np.float64)
    cc = (Cg * Cg).sum(1)
    rf2 = cc - bounds[:, 3].astype(np.float64)
    group_of = np.full(sc.n, -1, dtype=np.int64)
    rf_members = np.zeros(len(orig))
    for g in range(len(orig)):
        m = orig[g][orig[g] != 0xFFFFFFFF].astype(np.int64)
        group_of[m] = g
        if len(m):
            rf_members[g] = (np.linalg.norm(c[m] - Cg[g], axis=1) + r[m]).max()
    ok = (rf2 > 0) & (cc < 1e4 * np.maximum(rf2, 1e-300))
    return group_of, Cg, np.where(ok, np.sqrt(np.maximum(rf2, 0.0)), rf_members), orig


# ------------------------------------------------------------------------------------------------ small helpers
def centres(sc):
    return np.stack([sc.spheres["cx"], sc.spheres["cy"], sc.spheres["cz"]], 1).astype(np.float64)


def radii(sc):
    return np.abs(sc.spheres["r"].astype(np.float64))


def _unit(rng, m):
    v = rng.normal(size=(m, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(u, rng):
    """a random unit vector perpendicular to each row of u"""
    v = _unit(rng, len(u))
    w = v - (v * u).sum(1, keepdims=True) * u
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def _lengths(rng, m):
    return rng.choice(LENGTHS, m)[:, None]


def _pack(o, d):
    return np.concatenate([o, d], 1).astype(F)


def _exact_grid(values, magnitude):
    """values rounded to a multiple of a power of two q such that every multiple of q up to `magnitude` is a binary32 with four bits
    to spare: sums and differences of such numbers are exact."""
    q = 2.0 ** (np.ceil(np.log2(magnitude)) - 19)
    return np.round(np.asarray(values, dtype=np.float64) / q) * q


# ------------------------------------------------------------------------------------------------ scenes
def _base(spec, rng, n):
    """n base spheres in unit coordinates, the floor (soup, layer) last among them."""
    E = spec["extent"]
    if spec["layout"] == "box":
        # radii over three decades, six in ten of them in the top quarter [0.27, 1]: the layout gives every sphere above four times the
        # median radius a group of its own, and 509 or 512 spheres are a flat scan (128 groups of four) only when there is none
        c = rng.uniform(-E, E, (n, 3))
        r = np.where(rng.random(n) < 0.6, np.exp(rng.uniform(np.log(0.27), np.log(1.0), n)), np.exp(rng.uniform(np.log(1e-3), np.log(0.27), n)))
        return c, r, False
    if spec["layout"] == "soup":
        c = rng.uniform(-E, E, (n - 1, 3))
        c[:, 1] = np.abs(c[:, 1]) * 0.25
        r = np.exp(rng.uniform(np.log(0.05), np.log(1.2), n - 1))
        return np.concatenate([c, [[0.0, -401.5, 0.0]]]), np.concatenate([r, [400.0]]), True
    c = np.stack([rng.uniform(-E, E, n - 1), 0.2 + rng.uniform(0, 0.05, n - 1), rng.uniform(-E, E, n - 1)], 1)
    r = 0.2 * rng.uniform(0.5, 1.0, n - 1)
    return np.concatenate([c, [[0.0, -1000.0, 0.0]]]), np.concatenate([r, [1000.0]]), True


BIAS_RADII = (3e-4, 4e-4, 8e-4, 1.2e-3, 2e-3, 3e-3)  # absolute: the first two have a diameter below the bias
ROW_SPHERES = 120


def _make(oracle, spec, z0_hint=None):
    """The scene of a spec.  List order: the B spheres of half the near-equal pairs, the first members of the mirror pairs, the base
    spheres (floor last), the row, the bias spheres, the duplicates, the second members of the mirror pairs, the other B spheres.
    `n` counts them all."""
    rng = np.random.default_rng(spec["seed"])
    n, E, scale = spec["n"], spec["extent"], spec["scale"]
    off = np.asarray(spec["offset"], dtype=np.float64)
    layer = spec["layout"] == "layer"
    n_pairs = 4 if n < 37 else 8
    n_bias = 0 if n < 37 else len(BIAS_RADII)
    n_row = ROW_SPHERES if (n >= 400 and not layer) else 0
    n_dup, n_mirror = (6, 8) if spec["ties"] else (0, 0)
    n_base = n - n_pairs - n_bias - n_row - n_dup - 2 * n_mirror
    assert n_base >= 1
    c, r, floor = _base(spec, rng, n_base)
    n_small = n_base - (1 if floor else 0)
    if n_small == 1:  # flat5: the one base sphere carries all four pairs
        c[0], r[0] = (0.7, -0.4, 1.1), 0.8
    if spec["negative"]:
        sign = np.where(np.arange(n_base) % 3 == 0, -1.0, 1.0)
        if floor:
            sign[-1] = 1.0
        r = r * sign
    # the row: equal spheres along a slanted line through the box
    row = None
    if n_row:
        e_row = np.array([1.0, 0.03, 0.2])
        e_row /= np.linalg.norm(e_row)
        y0 = 0.45 * E if spec["layout"] == "box" else 0.35 * E * 0.25 + 1.0
        p0 = np.array([-0.85 * E, y0, -0.2 * E])
        step = 1.7 * E / ROW_SPHERES
        r_row = 0.3 if spec["layout"] == "box" else 0.3 * step  # (box: not below the top quarter of the radii, see _base)
        c = np.concatenate([c, p0 + np.arange(ROW_SPHERES)[:, None] * step * e_row])
        r = np.concatenate([r, np.full(ROW_SPHERES, r_row)])
        row = (p0 * scale + off, e_row, ROW_SPHERES * step * scale, r_row * scale)
    # to final coordinates; the bias spheres' radii are absolute
    c, r = c * scale + off, r * scale
    if n_bias:
        cb = rng.uniform(-0.6 * E, 0.6 * E, (n_bias, 3))
        if floor:
            cb[:, 1] = rng.uniform(0.5, 1.5, n_bias) if not layer else rng.uniform(0.6, 0.9, n_bias)
        c = np.concatenate([c, cb * scale + off])
        r = np.concatenate([r, BIAS_RADII])
    c, r = c.astype(F).astype(np.float64), r.astype(F).astype(np.float64)  # what the scene will hold
    Ef = E * scale
    # duplicates of base spheres of ordinary size
    order = np.argsort(np.abs(r[:n_small]))
    usable = order[len(order) // 2:] if n_small > 1 else order
    early = usable[usable < n_small // 2]  # the copy goes to the end of the list: a distant index
    dup_of = rng.choice(early, n_dup, replace=False) if n_dup else np.zeros(0, dtype=np.int64)
    # mirror pairs about z = z0: for the cell grid z0 is a border between two cells
    mirror_c = np.zeros((0, 3))
    mirror_r = np.zeros(0)
    z0 = None
    if n_mirror:
        # the members of a pair are 2 h apart and overlap in a lens of radius sqrt(r^2 - h^2) about the plane
        r_m = (0.19 if layer else 0.9) * scale
        z0 = off[2] + 0.37 * Ef if z0_hint is None else z0_hint
        mag = abs(z0) + 4.0 * r_m
        z0 = float(_exact_grid(z0, mag))
        h = float(_exact_grid((0.5 if layer else 0.9) * r_m, mag))
        assert h > 0 and F(z0 + h) == z0 + h and F(z0 - h) == z0 - h
        xs = off[0] + np.linspace(-0.7, 0.7, n_mirror) * Ef
        ys = off[1] + (np.full(n_mirror, 0.21) if layer else (rng.uniform(0.5, 3.0, n_mirror) if floor else rng.uniform(-0.5, 0.5, n_mirror) * Ef))
        first = np.stack([xs, ys, np.full(n_mirror, z0 + h)], 1)
        second = first.copy()
        second[:, 2] = z0 - h
        mirror_c = np.concatenate([first, second]).astype(F).astype(np.float64)
        mirror_r = np.full(2 * n_mirror, r_m).astype(F).astype(np.float64)
        assert np.array_equal(mirror_c[:n_mirror, :2], mirror_c[n_mirror:, :2])
    # near-equal pairs: A a base sphere, B with its top D above (D > 0) or below A's top along w
    pick_a = usable
    if spec["layout"] == "box" and n in (509, 512):  # B may be 2.5 times A and must not become a big sphere of the layout
        mid = np.nonzero((np.abs(r[:n_small]) >= 0.27 * scale) & (np.abs(r[:n_small]) <= 0.39 * scale))[0]
        pick_a = mid if len(mid) >= n_pairs else usable
    pa = rng.choice(pick_a, n_pairs, replace=len(pick_a) < n_pairs)  # (flat5: its one A)
    w = _unit(rng, n_pairs)
    if floor:
        w[:, 1] = 0.4 + np.abs(w[:, 1])
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    ra = np.abs(r[pa])
    ulp = np.spacing(np.abs(c[pa]).max(axis=1).astype(F)).astype(np.float64)
    # a small B stands D out of A (nearer at the top, farther off it: both orders around the circle where the surfaces cross);
    # a large B stays D below A's top (farther at the top, nearer off it).  flat5 has one A: small ones only there.  Outside the two
    # full flat scans a large B is also more than four times the median radius: the layout then gives it a group of its own (the
    # hierarchy and the grid test such a sphere apart from its neighbour A, with the far limit of whichever they found first).
    small_b = (np.arange(n_pairs) % 2 == 0) | (n_small == 1)
    D = np.maximum(ra * 2.0 ** -9, 8.0 * ulp) * np.where(small_b, 1.0, -1.0)
    rho_large = 2.5 * ra if (spec["layout"] == "box" and n in (509, 512)) else np.maximum(2.5 * ra, 4.5 * np.median(np.abs(r)))
    rho = np.where(small_b, 0.2 * ra, rho_large)
    cB = (c[pa] + (ra + D - rho)[:, None] * w).astype(F).astype(np.float64)
    rho = rho.astype(F).astype(np.float64)
    front = np.arange(n_pairs) % 4 < 2  # B before A in the list; with D's alternation: all four (nearer, earlier) combinations
    # assemble
    parts_c = [cB[front], mirror_c[:n_mirror], c, c[dup_of], mirror_c[n_mirror:], cB[~front]]
    parts_r = [rho[front], mirror_r[:n_mirror], r, r[dup_of], mirror_r[n_mirror:], rho[~front]]
    cc, rr = np.concatenate(parts_c), np.concatenate(parts_r)
    assert len(rr) == n
    starts = np.cumsum([0] + [len(p) for p in parts_r])
    b0 = int(starts[2])  # index of base sphere 0
    types = rng.choice([0, 0, 0, 1, 2, 3], n)
    if floor:
        types[b0 + n_base - 1] = 0
    centre = off + (np.array([0.0, 0.125 * Ef, 0.0]) if floor else 0.0)
    cam_o = centre + np.array([1.1, 0.45, -0.9]) * Ef * (0.5 if layer else 1.0)
    cam_l = centre + np.array([0.0, 0.0, 0.0])
    if layer:
        cam_o, cam_l = off + np.array([9.0, 1.2, -6.0]), off + np.array([0.0, 0.2, 0.0])
    sc = _scene(oracle, cc.astype(F), rr.astype(F), types, cam_o, cam_l, 45.0, 1.5, float(np.linalg.norm(cam_o - cam_l)), 0.0, rng)
    m = dict(extent=Ef, centre=off, floor=floor, layer=layer, scale=scale, row=row, z0=z0)
    m["floor_index"] = b0 + n_base - 1 if floor else -1
    m["bias"] = np.arange(b0 + len(c) - n_bias, b0 + len(c))
    m["dups"] = [(b0 + int(k), int(starts[3]) + j) for j, k in enumerate(dup_of)]
    m["mirrors"] = [(int(starts[1]) + j, int(starts[4]) + j) for j in range(n_mirror)]
    ib = np.zeros(n_pairs, dtype=np.int64)
    ib[front] = int(starts[0]) + np.arange(front.sum())
    ib[~front] = int(starts[5]) + np.arange((~front).sum())
    m["pairs"] = [(b0 + int(pa[j]), int(ib[j]), w[j]) for j in range(n_pairs)]
    m["base"] = np.arange(b0, b0 + n_small)
    sc.meta = m
    return sc


@functools.lru_cache(maxsize=None)
def _scene_of(oracle, name):
    c = case(name)
    with environment(c.env):
        sc = _make(oracle, c.spec)
        g = grid_info(sc.spheres)
        if g is not None and c.spec["ties"]:  # the mirror plane onto a border between two cells, the members into different cells
            nu, nv, au, av, gu, gv, inv = g[:7]
            assert 2 in (au, av)
            org, cells = (gv, nv) if av == 2 else (gu, nu)
            sc = _make(oracle, c.spec, z0_hint=org + round(0.62 * cells) / inv)
        return sc


def scene(oracle, name):
    """The scene of a case (built under the case's knobs: the cell-grid scene asks the layout for its cell borders)."""
    return _scene_of(oracle, "flat509_ties" if name.startswith("valu") else name)


# ------------------------------------------------------------------------------------------------ rays
class Rays:
    """classes: label -> [m, 6] binary32; meta: label -> what the honesty tests need (the aimed sphere of each ray, ...)."""

    def __init__(self):
        self.classes, self.meta = {}, {}

    def add(self, label, rays, **meta):
        assert rays.dtype == F and rays.shape[1] == 6
        self.classes[label], self.meta[label] = rays, meta

    def all(self):
        return np.ascontiguousarray(np.concatenate(list(self.classes.values())))

    def slice_of(self, label):
        at = 0
        for k, v in self.classes.items():
            if k == label:
                return slice(at, at + len(v))
            at += len(v)
        raise KeyError(label)


def _aimed(sc, rng, count, with_bias=True):
    """spheres the directed classes aim at: spread over the radii, the bias spheres among them, never the floor"""
    m = sc.meta
    pool = np.array([k for k in range(sc.n) if k != m["floor_index"]])
    pick = rng.choice(pool, min(count, len(pool)), replace=False)
    if with_bias and len(m["bias"]):
        pick = np.unique(np.concatenate([pick, m["bias"]]))
    return pick


def _grazers(sc, rng, m):
    meta = sc.meta
    c, r, E = centres(sc), radii(sc), meta["extent"]
    aim = _aimed(sc, rng, 40)
    k = aim[rng.integers(0, len(aim), m)]
    where = rng.choice(4, m, p=[0.45, 0.15, 0.25, 0.15])
    # from 10 extents away binary32 decides only for the smaller spheres: those rays aim at the smallest third
    smallest = aim[np.argsort(r[aim])][:max(1, len(aim) // 3)]
    k = np.where(where == 1, smallest[rng.integers(0, len(smallest), m)], k)
    u = _unit(rng, m)
    if meta["floor"]:
        u[:, 1] = -np.abs(u[:, 1])  # travelling downwards: the origin is above the closest approach
    w = _perp(u, rng)
    delta = 10.0 ** rng.uniform(GRAZE_K[0], GRAZE_K[1], m) * rng.choice([-1.0, 1.0], m)
    q = c[k] + (r[k] * (1.0 + delta))[:, None] * w
    s = np.where(where == 0, rng.uniform(0.5, 4.0, m) * r[k], np.array([0.0] + list(FAR))[where] * E * rng.uniform(0.7, 1.0, m))
    return _pack(q - s[:, None] * u, u * _lengths(rng, m)), dict(sphere=k, delta=delta, where=where)


def _ulp_along(p32, nrm, j):
    """p32 moved j ulp (of its largest component) along nrm, rounded to binary32 again"""
    ulp = np.spacing(np.abs(p32).max(axis=1)).astype(np.float64)
    return (p32.astype(np.float64) + (j * ulp)[:, None] * nrm).astype(F)


def _starters(sc, rng, m):
    meta = sc.meta
    c, r = centres(sc), radii(sc)
    aim = _aimed(sc, rng, 40)
    if meta["floor"]:
        aim = np.concatenate([aim, [meta["floor_index"]]])
    m_a = m // 2
    k = aim[rng.integers(0, len(aim), m_a)]
    nrm = _unit(rng, m_a)
    if meta["floor"]:
        fl = k == meta["floor_index"]
        up = np.stack([rng.uniform(-1, 1, m_a) * meta["extent"], np.zeros(m_a), rng.uniform(-1, 1, m_a) * meta["extent"]], 1) + meta["centre"]
        up = up - c[meta["floor_index"]]
        nrm[fl] = (up / np.linalg.norm(up, axis=1, keepdims=True))[fl]
    p = _ulp_along((c[k] + r[k][:, None] * nrm).astype(F), nrm, rng.choice([0, 0, 1, -1, 4, -4], m_a))
    tang = _perp(nrm, rng)
    eps = 10.0 ** rng.uniform(-6, -2, m_a) * rng.choice([-1.0, 1.0], m_a)
    d = tang + eps[:, None] * nrm
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    generic = _pack(p.astype(np.float64), d * _lengths(rng, m_a))
    # inward chords with the second root at the bias
    rs = r.astype(F).astype(np.float64)
    ok = np.nonzero((rs >= 5e-4) & (rs <= 4e-3))[0]
    if len(ok) == 0:
        return generic, dict(sphere=k, n_generic=m_a, target=np.zeros(0))
    m_b = m - m_a
    kb = ok[rng.integers(0, len(ok), m_b)]
    nb = _unit(rng, m_b)
    pb = _ulp_along((c[kb] + rs[kb][:, None] * nb).astype(F), nb, rng.choice([0, 0, 1, -1, 4, -4], m_b)).astype(np.float64)
    oc = pb - c[kb]
    ocn = np.linalg.norm(oc, axis=1)
    at_centre = ocn == 0  # (far from the origin a tiny sphere's surface point can round to its centre)
    ocn = np.where(at_centre, 1.0, ocn)
    nh = np.where(at_centre[:, None], nb, oc / ocn[:, None])
    tb = _perp(nh, rng)
    steps = rng.choice([0, 0, 1, -1, 8, -8], m_b)
    T = np.array([BIAS], dtype=F).repeat(m_b)
    for _ in range(8):
        T = np.where(steps > 0, np.nextafter(T, F(1)), T)
        T = np.where(steps < 0, np.nextafter(T, F(0)), T)
        steps = steps - np.sign(steps)
    T = T.astype(np.float64) * (1.0 + rng.choice([0.0, 0.0, 0.0, 1e-3, -1e-3], m_b))
    cq = ocn * ocn - rs[kb] * rs[kb]
    sphi = (T * T + cq) / (2.0 * T * ocn)  # T^2 + 2 b T + c = 0 with b = -|oc| sin(phi), |d| = 1
    good = (np.abs(sphi) < 1.0) & ~at_centre
    sphi = np.clip(sphi, -0.999, 0.999)
    db = np.sqrt(1.0 - sphi * sphi)[:, None] * tb - sphi[:, None] * nh
    chords = _pack(pb[good], db[good])
    return np.concatenate([generic, chords]), dict(sphere=np.concatenate([k, kb[good]]), n_generic=m_a, target=T[good])


def _behind(sc, rng, m):
    """Rays all but tangent to a group bound of rt_unit_layout (centre C, radius Rf): the normalised b = d.(o - C) / |o - C| is
    +-[1e-6, 1e-2].  The stored Rf carries the filter's margin, so the members of a group end mu Rf short of its surface (mu is 1e-3 to
    1e-2 in these scenes, 0.99 at the 2e4 offset), and a ray that flat touches only what lies within b^2 / 2 of its own distance from
    C: from (1 + delta) Rf it can hit a member only if delta <= -(mu - b^2 / 2).  Two halves:
      edge   a point Q on the cap of the member that reaches farthest out, a root s just beyond the bias (|d| = 0.3: s from 0.00033),
             the wanted b, and the origin o = Q - s d that has it -- placed so that the origin lies e times the members' reach below
             that reach, e log-uniform in [1e-7, 1e-2]: the rays that hit from as close to the bound's surface as its members allow;
      shell  origins at (1 + delta) Rf, delta = +-[1e-7, 1e-2], aimed along the tangent towards where that member touches: none of
             them can hit the group (the honesty test asserts it), the device must still not lose what lies behind it."""
    c, r, E = centres(sc), radii(sc), sc.meta["extent"]
    group_of, Cg, Rf, orig = group_bounds(sc)
    far, reach = np.full(len(Rf), -1), np.zeros(len(Rf))
    for gi in range(len(Rf)):
        mem = orig[gi][orig[gi] != 0xFFFFFFFF].astype(np.int64)
        if len(mem):
            out = np.linalg.norm(c[mem] - Cg[gi], axis=1) + r[mem]
            far[gi], reach[gi] = mem[np.argmax(out)], out.max()
    mu = 1.0 - reach / np.maximum(Rf, 1e-300)
    groups = np.nonzero((far >= 0) & (Rf < 4.0 * E) & (reach >= 0.0025) & (mu > 0))[0]
    if len(groups) == 0:
        groups = np.nonzero((far >= 0) & (mu > 0))[0]
    groups = groups[np.argsort(mu[groups])][:40]  # the tightest bounds
    g = groups[rng.integers(0, len(groups), m)]
    km = far[g]
    e = c[km] - Cg[g]
    en = np.linalg.norm(e, axis=1)
    e = np.where((en > 1e-9 * Rf[g])[:, None], e / np.maximum(en, 1e-300)[:, None], _unit(rng, m))
    length = np.where(rng.random(m) < 0.6, 0.3, rng.choice(LENGTHS, m))
    beta = 10.0 ** rng.uniform(-6, -2, m) * rng.choice([-1.0, 1.0], m)
    edge = np.arange(m) < m // 2
    # edge: the root s, then the cap angle psi that puts the origin e mu Rf below the members' reach
    s_lo = 0.0011 * length  # the root is s / |d|
    wide = rng.random(m) < 0.3
    s = np.exp(rng.uniform(np.log(s_lo), np.log(np.where(wide, np.maximum(2.0 * s_lo, 0.5 * reach[g]), 3.0 * s_lo))))
    s = np.minimum(s, 0.9 * reach[g])
    excess = 10.0 ** rng.uniform(-7, -2, m)
    beta = np.where(edge, np.sign(beta) * np.minimum(np.abs(beta), 0.5 * excess * reach[g] / s), beta)  # (a steeper ray cannot start that close)
    need = excess * reach[g] - s * s / (2.0 * reach[g]) - s * beta  # reach - |Q - C|
    psi = np.sqrt(np.clip(2.0 * reach[g] * need / np.maximum(en * r[km], 1e-300), 0.0, 1.0))
    nq = np.cos(psi)[:, None] * e + np.sin(psi)[:, None] * _perp(e, rng)
    Q = c[km] + r[km][:, None] * nq
    qv = Q - Cg[g]
    q = np.linalg.norm(qv, axis=1)
    Qh = qv / q[:, None]
    x = s / q
    for _ in range(40):  # (q x - s) = beta |o - C|, |o - C|^2 = q^2 - 2 q s x + s^2
        x = (s + beta * np.sqrt(np.maximum(q * q - 2.0 * q * s * x + s * s, 0.0))) / q
    x = np.clip(x, -0.999, 0.999)
    d = np.sqrt(1.0 - x * x)[:, None] * _perp(Qh, rng) + x[:, None] * Qh
    o = Q - s[:, None] * d
    # shell: on the sphere of radius (1 + delta) Rf, heading along the tangent with the slope beta
    delta_s = 10.0 ** rng.uniform(-7, -2, m) * rng.choice([-1.0, 1.0], m)
    tau = _perp(e, rng)
    back = np.exp(rng.uniform(np.log(0.002), np.log(0.3), m))  # the angle between the origin and the touching point
    wv = np.cos(back)[:, None] * e - np.sin(back)[:, None] * tau
    th = np.sin(back)[:, None] * e + np.cos(back)[:, None] * tau
    o = np.where(edge[:, None], o, Cg[g] + ((1.0 + delta_s) * Rf[g])[:, None] * wv)
    d = np.where(edge[:, None], d, np.sqrt(1.0 - beta * beta)[:, None] * th + beta[:, None] * wv)
    rays = _pack(o, d * length[:, None])
    rho = np.linalg.norm(rays[:, :3].astype(np.float64) - Cg[g], axis=1)  # of the origin as binary32 holds it
    return rays, dict(group=g, member=km, delta=rho / Rf[g] - 1.0, below=1.0 - rho / reach[g], beta=beta, mu=mu[g], reach=reach[g], edge=edge)


def _sag(radius, x):
    return radius - np.sqrt(radius * radius - x * x)


def _near_candidates(sc, rng, a, b, w, k, sign):
    """Rays down -w onto the tops of the pair (A, B), one per entry of k and sign: aimed at t_B - t_A = sign 2^-k t.  On the axis B's
    top is D above A's (as the scene holds the pair, after its rounding); at the distance x from it t_B - t_A = sag_B(x) - sag_A(x) - D.
    The origin 0.3 .. 1 R above the tops (at least 0.0045: the bias) is rounded to binary32 FIRST -- far from the origin of
    coordinates that moves it by a good part of x --, then the direction, a free binary32 vector, is laid through the point of A
    at the distance x from the axis.  Returns the rays that have such an x."""
    c, r = centres(sc), radii(sc)
    n = len(k)
    D = float((c[b] - c[a]) @ w + r[b]) - r[a]
    x_hi = 0.8 * min(r[a], r[b])
    grows = r[b] < r[a]  # B the smaller sphere: it falls away faster, t_B - t_A grows with x
    t = np.maximum(r[a] * rng.uniform(0.3, 1.0, n), 0.0045 * rng.uniform(1.0, 1.5, n))
    want = D + sign * t * 2.0 ** -k.astype(np.float64)  # = sag_B(x) - sag_A(x)
    lo, hi = np.zeros(n), np.full(n, x_hi)
    g_hi = _sag(r[b], x_hi) - _sag(r[a], x_hi)
    ok = (want >= 0) & (want <= g_hi) if grows else (want <= 0) & (want >= g_hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = (_sag(r[b], mid) - _sag(r[a], mid) < want) == grows
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    t, x, k = t[ok], lo[ok], k[ok]
    n = len(t)
    ww = np.repeat(w[None, :], n, 0)
    side = _perp(ww, rng) if n else np.zeros((0, 3))
    o = (c[a] + (r[a] + max(D, 0.0) + t)[:, None] * ww + side * x[:, None]).astype(F).astype(np.float64)
    lat = (o - c[a]) - ((o - c[a]) * ww).sum(1, keepdims=True) * ww
    ln = np.linalg.norm(lat, axis=1, keepdims=True)
    uh = np.where(ln > 0, lat / np.maximum(ln, 1e-300), side)
    d = c[a] + (r[a] - _sag(r[a], x))[:, None] * ww + x[:, None] * uh - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    return _pack(o, d * _lengths(rng, n)), k


NEAR_QUOTA = 12  # rays wanted per pair, side and measured gap 2^-15 .. 2^-24
NEAR_ROUNDS = 150


def _near(sc, rng, oracle):
    """Near-equal roots.  First 30 rays per pair, side and |eps| = 2^-9 .. 2^-14, as aimed.  Binary32 roots carry a few ulp of noise
    (2^-17 of the root far from the origin of coordinates), so the finer gaps are FOUND, not placed: rounds of 1,500 candidates per
    pair aimed at 2^-15 .. 2^-26, sorted by the gap the oracle's own two roots have, k = round(-log2 |t_B / t_A - 1|), and kept until
    every pair has NEAR_QUOTA of each side and each k = 15 .. 24 (at most NEAR_ROUNDS rounds)."""
    rays_out, ia, ib, kk = [], [], [], []

    def take(a, b, rays, k):
        rays_out.append(rays)
        ia.extend([a] * len(rays))
        ib.extend([b] * len(rays))
        kk.extend(k.tolist())

    one = oracle.Oracle()

    def roots(k_sphere, rays):
        one.upload(oracle.Scene(sc.spheres[k_sphere:k_sphere + 1], sc.materials[k_sphere:k_sphere + 1], sc.camera, sc.sun, sc.sky, sc.exposure_scale))
        h = one.closest_hit(rays)
        return np.where(h[:, 1].copy().view(np.int32) >= 0, h[:, 0].astype(np.float64), np.nan)

    try:
        for (a, b, w) in sc.meta["pairs"]:
            coarse_k = np.repeat(np.arange(9, 15), 2 * 30)
            coarse_s = np.tile(np.repeat([-1.0, 1.0], 30), 6)
            rays, k = _near_candidates(sc, rng, a, b, w, coarse_k, coarse_s)
            take(a, b, rays, k)
            have = {}
            for _ in range(NEAR_ROUNDS):
                m = 1500
                rays, k = _near_candidates(sc, rng, a, b, w, rng.integers(15, 27, m), rng.choice([-1.0, 1.0], m))
                if len(rays) == 0:
                    break
                ta, tb = roots(a, rays), roots(b, rays)
                with np.errstate(all="ignore"):
                    km = np.where(np.isfinite(ta) & np.isfinite(tb) & (ta != tb), np.rint(-np.log2(np.abs(tb / ta - 1.0))), -1).astype(np.int64)
                keep = np.zeros(len(rays), dtype=bool)
                for i in np.nonzero((km >= 15) & (km <= 24))[0]:
                    key = (int(km[i]), bool(tb[i] < ta[i]))
                    if have.get(key, 0) < NEAR_QUOTA:
                        have[key] = have.get(key, 0) + 1
                        keep[i] = True
                take(a, b, rays[keep], km[keep])
                if all(have.get((kq, sq), 0) >= NEAR_QUOTA for kq in range(15, 25) for sq in (False, True)):
                    break
    finally:
        one.close()
    return np.concatenate(rays_out), dict(a=np.array(ia), b=np.array(ib), k=np.array(kk))


def _ties(sc, rng, per_dup=150, per_mirror=190):
    meta = sc.meta
    c, r = centres(sc), radii(sc)
    out, first, second = [], [], []
    for (a, b) in meta["dups"]:
        v = _unit(rng, per_dup)
        if meta["floor"]:
            v[:, 1] = np.abs(v[:, 1])
        o = c[a] + (r[a] * rng.uniform(1.5, 4.0, per_dup))[:, None] * v
        target = c[a] + (r[a] * rng.uniform(0, 0.98, per_dup))[:, None] * _unit(rng, per_dup)
        d = target - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append(_pack(o, d * _lengths(rng, per_dup)))
        first += [a] * per_dup
        second += [b] * per_dup
    z0 = meta["z0"]
    for (a, b) in meta["mirrors"]:
        h = abs(c[a][2] - z0)
        lens = np.sqrt(r[a] ** 2 - h ** 2)
        ang = rng.uniform(0, np.pi, per_mirror) if meta["floor"] else rng.uniform(0, 2 * np.pi, per_mirror)
        dist = r[a] * rng.uniform(1.5, 4.0, per_mirror)
        o = np.stack([c[a][0] + dist * np.cos(ang), c[a][1] + dist * np.sin(ang), np.full(per_mirror, z0)], 1)
        ja = rng.uniform(0, 2 * np.pi, per_mirror)
        jr = lens * np.sqrt(rng.uniform(0, 0.8, per_mirror))
        target = np.stack([c[a][0] + jr * np.cos(ja), c[a][1] + jr * np.sin(ja), np.full(per_mirror, z0)], 1)
        d = target - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d = d * _lengths(rng, per_mirror)
        d[:, 2] = 0.0
        rays = _pack(o, d)
        assert (rays[:, 2] == F(z0)).all() and (rays[:, 5] == 0).all()
        out.append(rays)
        first += [a] * per_mirror
        second += [b] * per_mirror
    return np.concatenate(out), dict(first=np.array(first), second=np.array(second))


TINY = (0.0, -0.0, 1e-30, -1e-30, 1e-40, -1e-40)  # +0, -0, tiny normals, denormals


def _box(sc):
    """the box around the spheres that are not the floor"""
    c, r = centres(sc), radii(sc)
    keep = np.arange(sc.n) != sc.meta["floor_index"]
    return (c[keep] - r[keep, None]).min(0), (c[keep] + r[keep, None]).max(0)


def _degenerate(sc, rng, per_dir=6):
    meta = sc.meta
    c, r = centres(sc), radii(sc)
    lo, hi = _box(sc)
    pool = np.array([k for k in range(sc.n) if k != meta["floor_index"]])
    borders = None
    g = grid_info(sc.spheres)
    if g is not None:
        nu, nv, au, av, gu, gv, inv = g[:7]
        borders = {au: gu + np.arange(nu + 1) / inv, av: gv + np.arange(nv + 1) / inv}
    dirs = []
    for axis in range(3):
        for sgn in (1.0, -1.0):
            for t1 in TINY:
                for t2 in TINY:
                    d = np.zeros(3)
                    d[axis] = sgn
                    d[(axis + 1) % 3], d[(axis + 2) % 3] = t1, t2
                    dirs.append((axis, d))
    o_all, d_all, kinds = [], [], []
    for axis, d in dirs:
        k = pool[rng.integers(0, len(pool), per_dir)]
        o = c[k] + (r[k] * rng.uniform(-0.9, 0.9, per_dir))[:, None] * _unit(rng, per_dir)  # the line passes through sphere k
        kind = rng.integers(0, 4, per_dir)
        span = hi[axis] - lo[axis]
        along = np.where(d[axis] > 0, lo[axis] - rng.uniform(0.2, 1.5, per_dir) * span, hi[axis] + rng.uniform(0.2, 1.5, per_dir) * span)  # outside
        along = np.where(kind == 1, rng.uniform(lo[axis], hi[axis], per_dir), along)  # inside
        face = np.where(rng.random(per_dir) < 0.5, lo[axis], hi[axis])
        along = np.where(kind == 2, face, along)  # on a face of the box
        o[:, axis] = along
        o = o.astype(F)
        other = (axis + 1) % 3
        if borders is not None and other in borders:  # kind 3: on a cell border across the ray
            on = kind == 3
            o[on, other] = borders[other][rng.integers(0, len(borders[other]), on.sum())].astype(F)
        for col, sel in ((axis, kind == 2), (other, kind == 3)):
            for _ in range(4):  # +-4 ulp
                step = sel & (rng.random(per_dir) < 0.5)
                up = rng.random(per_dir) < 0.5
                o[:, col] = np.where(step, np.nextafter(o[:, col], np.where(up, F(np.inf), F(-np.inf)).astype(F)), o[:, col])
        o_all.append(o)
        d_all.append(np.repeat((d * rng.choice(LENGTHS))[None, :], per_dir, 0))
        kinds.append(kind)
    # one component exactly zero, the others ordinary
    m2 = 400
    d2 = _unit(rng, m2)
    d2[np.arange(m2), rng.integers(0, 3, m2)] = rng.choice([0.0, -0.0], m2)
    k2 = pool[rng.integers(0, len(pool), m2)]
    o2 = c[k2] + (r[k2] * rng.uniform(-0.9, 0.9, m2))[:, None] * _unit(rng, m2) - d2 * (rng.uniform(0.1, 2.0, m2) * meta["extent"])[:, None]
    rays = np.concatenate([np.concatenate([np.concatenate(o_all).astype(F), np.concatenate(d_all).astype(F)], 1), _pack(o2, d2)])
    return rays, dict(kind=np.concatenate(kinds + [np.full(m2, 4)]))


def _crowded(sc, rng, waves=10):
    """waves x [64 crowded rays | 64 misses | 64 misses with one crowded ray]; meta crowded: the crowded waves' first rays."""
    meta = sc.meta
    E, ctr = meta["extent"], meta["centre"]

    def skim(m):
        if meta["row"] is not None:
            p0, e, length, rr = meta["row"]
            side = _perp(np.repeat(e[None, :], m, 0), rng)
            o = p0 - e * (rng.uniform(0.5, 2.0, m) * 4 * rr)[:, None] + side * (rng.uniform(0, 1.3, m) * rr)[:, None]
            aim = p0 + e * length + side * (rng.uniform(-1.3, 1.3, m) * rr)[:, None]
            d = aim - o
        elif meta["layer"]:
            ang = rng.uniform(0, 2 * np.pi, m)
            e = np.stack([np.cos(ang), np.zeros(m), np.sin(ang)], 1)
            through = ctr + np.stack([rng.uniform(-0.5, 0.5, m) * E, 0.2 + rng.uniform(0.0, 0.12, m), rng.uniform(-0.5, 0.5, m) * E], 1)
            o = through - e * 1.6 * E
            d = e + np.stack([np.zeros(m), rng.uniform(-1e-3, 1e-3, m), np.zeros(m)], 1)
        else:
            e = _unit(rng, m)
            o = ctr + rng.uniform(-0.3, 0.3, (m, 3)) * E - e * 2.0 * E
            d = e
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        return o, d * _lengths(rng, m)

    def miss(m):
        v = _unit(rng, m)
        v[:, 1] = np.abs(v[:, 1]) + 0.2
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return ctr + v * 3.0 * E, v * _lengths(rng, m)

    blocks, starts, at = [], [], 0
    for _ in range(waves):
        o, d = skim(64)
        blocks.append(_pack(o, d))
        starts.append(at)
        o, d = miss(64)
        blocks.append(_pack(o, d))
        o, d = miss(64)
        o1, d1 = skim(1)
        lane = int(rng.integers(0, 64))
        o[lane], d[lane] = o1[0], d1[0]
        blocks.append(_pack(o, d))
        at += 192
    return np.concatenate(blocks), dict(crowded=np.array(starts))


@functools.lru_cache(maxsize=None)
def _rays_of(oracle, name, seed):
    sc = scene(oracle, name)
    rng = np.random.default_rng(seed)
    R = Rays()
    with environment(case(name).env):  # the group bounds and the cell grid are those of the case's knobs
        for label, fn, arg in (("grazers", _grazers, 21000), ("starters", _starters, 4000), ("behind", _behind, 1500)):
            rays, meta = fn(sc, rng, arg)
            R.add(label, rays, **meta)
        rays, meta = _near(sc, rng, oracle)
        R.add("near", rays, **meta)
        if sc.meta["dups"]:
            rays, meta = _ties(sc, rng)
            R.add("ties", rays, **meta)
        rays, meta = _degenerate(sc, rng)
        R.add("degenerate", rays, **meta)
        rays, meta = _crowded(sc, rng)
        R.add("crowded", rays, **meta)
    return R


def rays(oracle, name, seed=None):
    """The rays of a case's scene as labelled classes (a Rays); a multiple of 64 up to the crowded class, whose waves are then waves of
    the launch too, plus 37 random rays at the end: the count is no multiple of 256 or of 64."""
    name = "flat509_ties" if name.startswith("valu") else name
    return _rays_of(oracle, name, case(name).spec["seed"] + 50 if seed is None else seed)


def all_rays(oracle, name):
    """Every ray of the case in launch order: the classes before `crowded` padded with random rays to a multiple of 64, the crowded
    class, 37 random rays."""
    R = rays(oracle, name)
    sc = scene(oracle, name)
    rng = np.random.default_rng(case(name).spec["seed"] + 99)
    E, ctr = sc.meta["extent"], sc.meta["centre"]

    def random_rays(m):
        o = ctr + rng.uniform(-1.5, 1.5, (m, 3)) * E
        return _pack(o, _unit(rng, m) * _lengths(rng, m))

    head = np.concatenate([v for k, v in R.classes.items() if k != "crowded"])
    pad = random_rays((-len(head)) % 64)
    out = np.concatenate([head, pad, R.classes["crowded"], random_rays(37)])
    return np.ascontiguousarray(out), len(head) + len(pad)


# ------------------------------------------------------------------------------------------------ the oracle, one sphere at a time
def own_sphere_hits(oracle, sc, sphere, rays):
    """[m, 10]: the oracle's record of each ray against sphere[i] ALONE (a one-sphere scene through the list scan)."""
    rays = np.ascontiguousarray(rays, dtype=F)
    out = np.zeros((len(rays), 10), dtype=F)
    one = oracle.Oracle()
    try:
        for k in np.unique(sphere):
            sel = np.nonzero(sphere == k)[0]
            one.upload(oracle.Scene(sc.spheres[k:k + 1], sc.materials[k:k + 1], sc.camera, sc.sun, sc.sky, sc.exposure_scale))
            out[sel] = one.closest_hit(rays[sel])
    finally:
        one.close()
    return out


def without(oracle, sc, k):
    """the scene minus sphere k"""
    keep = np.arange(sc.n) != k
    return oracle.Scene(sc.spheres[keep], sc.materials[keep], sc.camera, sc.sun, sc.sky, sc.exposure_scale)
