"""The recipes of the trace-kernel census (tests/test_trace_variants_cpu.py, tests/test_trace_variants.py): plain data and scene builders.

librt_hip.so instantiates the 55 rows of csrc/rt_trace_variants.h, each as rt_trace_kernel<...> and as its rt_trace_kernel_lights<...>
twin, and host/rt_launch_plan.cpp picks one per launch from the scene's shape, the context's settings and the RT_* knobs.  A recipe is
one way to make a real upload and a real render land on one of the 110: a scene, a light list, the environment of rt_create, the upload
and the launch, the mode, and the kernel word (word [25] of rt_unit_launch_plan, include/rt_api.h) that the launcher must then report.

The scenes: the stock `cover` (488 spheres: the flat matrix-core scan; the cell grid under RT_GRID=2) and `grid10k` (10,004 spheres: the
cell grid; the bounds hierarchy under RT_GRID=0), and two seeded generated layers of small spheres over the big floor sphere:
`small300`, small enough that the all-in-LDS cell-grid kernel keeps room for its path caches, and `cells53k`, whose grid under
RT_GRID_DENSITY=0.1 has more cells than LDS holds.  Every scene has glass, metal, emissive and checker materials and the floor, so that hit processing of every
class, shadow queries and far hit points all occur (the CPU census asserts it)."""
import collections
import ctypes as C

import numpy as np

# --------------------------------------------------------------------------------------------------------- kernel words
_THREADS = {256: 0, 512: 1, 1024: 2}


def kernel_word(kLds, kThreads, kScan, kCache, kHitLds, kCarry=False, kStash=False, kMatsL2=False, kSgLds=False, kGridQ=False, lights=False):
    """Word [25] of rt_unit_launch_plan for an instantiated variant: the template arguments of rt_trace_kernel in the order of a row
    X(...) of csrc/rt_trace_variants.h, bit 0 the _lights twin, bit 31 set."""
    return ((1 if lights else 0) | (2 if kLds else 0) | _THREADS[kThreads] << 2 | kScan << 4 | (1 << 6 if kCache else 0) | (1 << 7 if kHitLds else 0) |
            (1 << 8 if kCarry else 0) | (1 << 9 if kStash else 0) | (1 << 10 if kMatsL2 else 0) | (1 << 11 if kSgLds else 0) |
            (1 << 12 if kGridQ else 0) | 1 << 31)


def twin(word, lights):
    return (word & ~1) | (1 if lights else 0)


# --------------------------------------------------------------------------------------------------------- scenes
SCENES = ("cover", "grid10k", "small300", "cells53k")
SECOND_LIGHT = ((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0)  # light 1 of test_light_list_images_equal_the_oracle's pool


def _layer(aspect, name, seed, n, side, r_small, cam_o):
    """n small spheres of every material class in a layer, and the floor: a scene for the cell grid.  Built the way
    test_random_scenes_differential builds its soups: a seeded generator, byte colours, the oracle's camera."""
    from oracle import oracle_py as O
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-side, side, n), rng.uniform(-side, side, n)
    r = r_small * rng.uniform(0.5, 1.0, n)
    centers = np.concatenate([np.stack([a, r + rng.uniform(0.0, 0.05, n), b], 1), [[0.0, -1000.0, 0.0]]]).astype(np.float32)
    radii = np.concatenate([r, [1000.0]]).astype(np.float32)
    types = np.concatenate([rng.choice([0, 0, 1, 2, 3], n), [0]]).astype(np.uint32)
    n += 1
    sph = np.zeros(n, dtype=O.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"], sph["r"] = centers[:, 0], centers[:, 1], centers[:, 2], radii
    mat = np.zeros(n, dtype=O.MATERIAL_DTYPE)
    k255 = np.float32(1) / np.float32(255)
    mat["type"] = types
    mat["tex_type"] = rng.integers(0, 2, n)
    mat["tex_type"][n - 1] = 1  # the floor is a checker
    mat["tiling"] = rng.choice([4.0, 50.0], n)
    mat["tiling"][n - 1] = 2500.0
    mat["rgb0"] = rng.integers(0, 256, (n, 3)).astype(np.float32) * k255
    mat["rgb1"] = rng.integers(0, 256, (n, 3)).astype(np.float32) * k255
    mat["smoothness"] = np.where(types == 1, 0.0, rng.uniform(1.0, 64.0, n)).astype(np.float32)
    mat["ior"] = rng.uniform(1.1, 2.4, n).astype(np.float32)
    mat["luminance"] = np.where(types == 3, rng.uniform(100.0, 20000.0, n), 0.0).astype(np.float32)
    ref = O.build_scene("three", 1, aspect)
    cam = O.RtCamera()
    o, la = np.asarray(cam_o, dtype=np.float64), np.array([0.0, 0.2, 0.0])
    O.lib().orc_camera_make((C.c_float * 3)(*o), (C.c_float * 3)(*la), 40.0, aspect, float(np.linalg.norm(o - la)), 0.05, C.byref(cam))
    return O.Scene(sph, mat, cam, ref.sun, ref.sky, ref.exposure_scale, name, seed)


# small300: about 300 scan entries, for the all-in-LDS cell grid (RT_GRID=2) with room left for its path caches.
# cells53k: 5,300 spheres of at most 10 cm over 100 x 100 units; under RT_GRID_DENSITY=0.1 the builder cuts cells of 0.43 units,
# about 232 x 232 = 53,800 of them (more than the 44,912 whose 2 bytes each fit LDS beside the grid scan's work lists; the builder's
# limits are 254 a side and 60,000 in all, and a cell of at least 2.5 radii -- which is why grid10k itself cannot get there).
_LAYERS = {"small300": (5302, 300, 7.0, 0.28, (10.0, 3.0, -8.0)), "cells53k": (5309, 5300, 50.0, 0.1, (40.0, 9.0, -30.0))}


def build_scene(name, W, H, n_lights=1):
    """The scene `name` for a W x H picture with its light list: 1 = the scene's own sun (no list attribute: the single-light kernels),
    2 = [sun, SECOND_LIGHT], 0 = the empty list (the twin, with no light to add)."""
    from oracle import oracle_py as O
    if name in _LAYERS:
        sc = _layer(W / float(H), name, *_LAYERS[name])
    else:
        from cpuraytracer_amd import scenes
        sc = scenes.build_scene(name, 1, W, H)
        # the stock generators make no emissive sphere: every eleventh diffuse one becomes a lamp
        lamps = np.flatnonzero(sc.materials["type"] == 0)[5::11]
        lamps = lamps[sc.spheres["r"][lamps] < 100.0]
        sc.materials["type"][lamps] = 3
        sc.materials["luminance"][lamps] = 3000.0
    if n_lights == 2:
        sc.lights = [sc.sun, O.make_light(*SECOND_LIGHT)]
    elif n_lights == 0:
        sc.lights = []
    else:
        assert n_lights == 1
    return sc


# --------------------------------------------------------------------------------------------------------- recipes
# mode: "ordinary", or ("carry", depth) = stats-less 1-spp frames under rt_set_frame_pipelining(depth).
# why_again: None, or the reason this recipe expects a kernel word that another recipe expects too.
Recipe = collections.namedtuple("Recipe", ["name", "row", "scene", "n_lights", "env", "mode", "kernel", "why_again"])

# One way to each row of csrc/rt_trace_variants.h: (row, scene, environment, the row's template arguments kLds, kThreads, kScan, kCache,
# kHitLds, kCarry, kStash, kMatsL2, kSgLds, kGridQ -- written out, not read from the library: the CPU census compares them with
# rt_unit_trace_variants).  The environment holds rt_create's settings (RT_SCAN, RT_BLOCK_THREADS, RT_BLOCKS_PER_CU, RT_MATS_LDS,
# RT_RAY_CACHE, RT_STASH, RT_TREE_LDS, RT_FORCE_GLOBAL_TABLES), the upload's (RT_GRID, RT_GRID_DENSITY) and the launch's knobs
# (RT_MATS_L2, RT_GRID_QUANT, RT_GRID_SG_LDS).  Found by sweeping host/rt_launch_plan.cpp over the shapes host/rt_scene_prep.cpp gives
# these scenes; what the device reports for them is in docs/EXPERIMENTS.md.
_ROWS = (
    ( 0, "cover",    {},                                                                                                      (True, 1024, 1, True, True, True, False, False, False, False)),
    ( 1, "cover",    {"RT_GRID": "2"},                                                                                       (True, 1024, 3, True, True, False, True, False, False, False)),
    ( 2, "small300", {"RT_GRID": "2", "RT_STASH": "0"},                                                                      (True, 1024, 3, True, True, False, False, False, False, False)),
    ( 3, "cover",    {"RT_GRID": "2", "RT_STASH": "0", "RT_RAY_CACHE": "0"},                                                 (True, 1024, 3, False, True, False, False, False, False, False)),
    ( 4, "cover",    {"RT_GRID": "2", "RT_FORCE_GLOBAL_TABLES": "1", "RT_GRID_SG_LDS": "1"},                                 (False, 1024, 3, True, True, False, True, False, True, False)),
    ( 5, "grid10k",  {"RT_GRID_QUANT": "1"},                                                                                 (False, 1024, 3, True, True, False, True, False, False, True)),
    ( 6, "grid10k",  {},                                                                                                     (False, 1024, 3, True, True, False, True, False, False, False)),
    ( 7, "grid10k",  {"RT_STASH": "0"},                                                                                      (False, 1024, 3, True, True, False, False, False, False, False)),
    ( 8, "grid10k",  {"RT_STASH": "0", "RT_RAY_CACHE": "0"},                                                                 (False, 1024, 3, False, True, False, False, False, False, False)),
    ( 9, "cells53k", {"RT_GRID_DENSITY": "0.1"},                                                                             (False, 1024, 3, False, False, False, False, False, False, False)),
    (10, "grid10k",  {"RT_BLOCK_THREADS": "512", "RT_RAY_CACHE": "0"},                                                       (False,  512, 3, False, False, False, False, False, False, False)),
    (11, "grid10k",  {"RT_BLOCK_THREADS": "512"},                                                                            (False,  512, 3, True, False, False, False, False, False, False)),
    (12, "grid10k",  {"RT_BLOCK_THREADS": "256", "RT_RAY_CACHE": "0"},                                                       (False,  256, 3, False, False, False, False, False, False, False)),
    (13, "grid10k",  {"RT_BLOCK_THREADS": "256"},                                                                            (False,  256, 3, True, False, False, False, False, False, False)),
    (14, "grid10k",  {"RT_GRID": "0"},                                                                                       (False, 1024, 2, True, True, False, True, False, False, False)),
    (15, "grid10k",  {"RT_GRID": "0", "RT_TREE_LDS": "0"},                                                                   (False, 1024, 2, True, False, False, True, False, False, False)),
    (16, "cover",    {},                                                                                                     (True, 1024, 1, True, True, False, True, True, False, False)),
    (17, "cover",    {"RT_MATS_L2": "0"},                                                                                    (True, 1024, 1, True, True, False, True, False, False, False)),
    (18, "cover",    {"RT_MATS_LDS": "0"},                                                                                   (True, 1024, 1, True, False, False, True, False, False, False)),
    (19, "grid10k",  {"RT_GRID": "0", "RT_STASH": "0"},                                                                      (False, 1024, 2, True, True, False, False, False, False, False)),
    (20, "grid10k",  {"RT_GRID": "0", "RT_STASH": "0", "RT_RAY_CACHE": "0"},                                                 (False, 1024, 2, False, True, False, False, False, False, False)),
    (21, "grid10k",  {"RT_GRID": "0", "RT_STASH": "0", "RT_TREE_LDS": "0"},                                                  (False, 1024, 2, True, False, False, False, False, False, False)),
    (22, "grid10k",  {"RT_GRID": "0", "RT_STASH": "0", "RT_RAY_CACHE": "0", "RT_TREE_LDS": "0"},                             (False, 1024, 2, False, False, False, False, False, False, False)),
    (23, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "512"},                                                            (False,  512, 2, True, True, False, False, False, False, False)),
    (24, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "512", "RT_RAY_CACHE": "0"},                                       (False,  512, 2, False, True, False, False, False, False, False)),
    (25, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "512", "RT_TREE_LDS": "0"},                                        (False,  512, 2, True, False, False, False, False, False, False)),
    (26, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "512", "RT_RAY_CACHE": "0", "RT_TREE_LDS": "0"},                   (False,  512, 2, False, False, False, False, False, False, False)),
    (27, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "256"},                                                            (False,  256, 2, True, True, False, False, False, False, False)),
    (28, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "256", "RT_RAY_CACHE": "0"},                                       (False,  256, 2, False, True, False, False, False, False, False)),
    (29, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "256", "RT_TREE_LDS": "0"},                                        (False,  256, 2, True, False, False, False, False, False, False)),
    (30, "grid10k",  {"RT_GRID": "0", "RT_BLOCK_THREADS": "256", "RT_RAY_CACHE": "0", "RT_TREE_LDS": "0"},                   (False,  256, 2, False, False, False, False, False, False, False)),
    (31, "cover",    {"RT_STASH": "0"},                                                                                      (True, 1024, 1, True, True, False, False, False, False, False)),
    (32, "cover",    {"RT_STASH": "0", "RT_RAY_CACHE": "0"},                                                                 (True, 1024, 1, False, True, False, False, False, False, False)),
    (33, "cover",    {"RT_STASH": "0", "RT_MATS_LDS": "0"},                                                                  (True, 1024, 1, True, False, False, False, False, False, False)),
    (34, "cover",    {"RT_STASH": "0", "RT_MATS_LDS": "0", "RT_RAY_CACHE": "0"},                                             (True, 1024, 1, False, False, False, False, False, False, False)),
    (35, "cover",    {"RT_BLOCK_THREADS": "512"},                                                                            (True,  512, 1, True, True, False, False, False, False, False)),
    (36, "cover",    {"RT_BLOCK_THREADS": "512", "RT_RAY_CACHE": "0"},                                                       (True,  512, 1, False, True, False, False, False, False, False)),
    (37, "cover",    {"RT_BLOCK_THREADS": "512", "RT_MATS_LDS": "0"},                                                        (True,  512, 1, True, False, False, False, False, False, False)),
    (38, "cover",    {"RT_BLOCK_THREADS": "512", "RT_MATS_LDS": "0", "RT_RAY_CACHE": "0"},                                   (True,  512, 1, False, False, False, False, False, False, False)),
    (39, "cover",    {"RT_BLOCK_THREADS": "256"},                                                                            (True,  256, 1, True, True, False, False, False, False, False)),
    (40, "cover",    {"RT_BLOCK_THREADS": "256", "RT_RAY_CACHE": "0"},                                                       (True,  256, 1, False, True, False, False, False, False, False)),
    (41, "cover",    {"RT_BLOCK_THREADS": "256", "RT_MATS_LDS": "0"},                                                        (True,  256, 1, True, False, False, False, False, False, False)),
    (42, "cover",    {"RT_BLOCK_THREADS": "256", "RT_MATS_LDS": "0", "RT_RAY_CACHE": "0"},                                   (True,  256, 1, False, False, False, False, False, False, False)),
    (43, "cover",    {"RT_SCAN": "valu", "RT_BLOCK_THREADS": "1024", "RT_BLOCKS_PER_CU": "1"},                               (True, 1024, 0, True, False, False, False, False, False, False)),
    (44, "cover",    {"RT_SCAN": "valu", "RT_BLOCK_THREADS": "1024", "RT_BLOCKS_PER_CU": "1", "RT_RAY_CACHE": "0"},          (True, 1024, 0, False, False, False, False, False, False, False)),
    (45, "cover",    {"RT_SCAN": "valu", "RT_BLOCK_THREADS": "512", "RT_BLOCKS_PER_CU": "1"},                                (True,  512, 0, True, False, False, False, False, False, False)),
    (46, "cover",    {"RT_SCAN": "valu", "RT_BLOCK_THREADS": "512", "RT_BLOCKS_PER_CU": "1", "RT_RAY_CACHE": "0"},           (True,  512, 0, False, False, False, False, False, False, False)),
    (47, "cover",    {"RT_SCAN": "valu", "RT_BLOCKS_PER_CU": "1"},                                                           (True,  256, 0, True, False, False, False, False, False, False)),
    (48, "cover",    {"RT_SCAN": "valu", "RT_BLOCKS_PER_CU": "1", "RT_RAY_CACHE": "0"},                                      (True,  256, 0, False, False, False, False, False, False, False)),
    (49, "cover",    {"RT_FORCE_GLOBAL_TABLES": "1"},                                                                        (False, 1024, 0, True, False, False, False, False, False, False)),
    (50, "cover",    {"RT_FORCE_GLOBAL_TABLES": "1", "RT_RAY_CACHE": "0"},                                                   (False, 1024, 0, False, False, False, False, False, False, False)),
    (51, "cover",    {"RT_FORCE_GLOBAL_TABLES": "1", "RT_BLOCK_THREADS": "512"},                                             (False,  512, 0, True, False, False, False, False, False, False)),
    (52, "cover",    {"RT_FORCE_GLOBAL_TABLES": "1", "RT_BLOCK_THREADS": "512", "RT_RAY_CACHE": "0"},                        (False,  512, 0, False, False, False, False, False, False, False)),
    (53, "grid10k",  {"RT_SCAN": "valu"},                                                                                    (False,  256, 0, True, False, False, False, False, False, False)),
    (54, "grid10k",  {"RT_SCAN": "valu", "RT_RAY_CACHE": "0"},                                                               (False,  256, 0, False, False, False, False, False, False, False)),
)
CARRY_DEPTH = 2
# Not reached by any recipe: (row, reason).  Both twins of a row; at most MAX_NOT_RUN rows.  Empty: every row is reached.
NOT_RUN = ()
MAX_NOT_RUN = 3
# The empty light list (n_lights == 0 takes the _lights twin, with no light to add and no shadow index): once per scan family
_EMPTY_LIST_ROWS = {48: "VALU scan", 16: "flat scan", 14: "hierarchy scan", 6: "cell-grid scan"}


def _recipes():
    out = []
    for row, scene, env, args in _ROWS:
        mode = ("carry", CARRY_DEPTH) if args[5] else "ordinary"
        for n_lights in (1, 2):
            out.append(Recipe("row%02d_%s_%s" % (row, scene, "sun" if n_lights == 1 else "two_lights"), row, scene, n_lights, dict(env), mode,
                              kernel_word(*args, lights=n_lights != 1), None))
        if row in _EMPTY_LIST_ROWS:
            out.append(Recipe("row%02d_%s_no_lights" % (row, scene), row, scene, 0, dict(env), mode, kernel_word(*args, lights=True),
                              "the empty light list takes the twin too: once per scan family (%s)" % _EMPTY_LIST_ROWS[row]))
    return tuple(out)


RECIPES = _recipes()


def recipe(name):
    return next(r for r in RECIPES if r.name == name)


def waves_per_cu(env):
    """Waves a CU holds under a recipe's settings, as rt_create reads them: blocks per CU x threads / 64."""
    valu = env.get("RT_SCAN") == "valu"
    return int(env.get("RT_BLOCKS_PER_CU", 4 if valu else 1)) * int(env.get("RT_BLOCK_THREADS", 256 if valu else 1024)) // 64
