"""The cases of tests/test_launch_plan_cpu.py: packed inputs of `rt_unit_launch_plan` (include/rt_api.h documents the words), a seeded
random part and a directed part.  tests/golden/launch_plans.npz holds what the launcher answered for exactly these cases BEFORE it
became host/rt_launch_plan.cpp (docs/EXPERIMENTS.md: how it was recorded), so this file must not change without re-recording it --
`cases_digest` in the fixture says whether it has.
"""
import hashlib

import numpy as np

CASE_WORDS = PLAN_WORDS = 28
FIELDS = ("n_padded", "n_levels", "top_cnt", "top_off", "shape_flags", "grid_nu", "grid_nv", "sg_nx", "sg_ny", "sg_nentries", "sg_nglobal",
          "n_lights", "cu_count", "blocks_per_cu", "block_threads", "setting_flags", "mats16", "mats_l2", "stash_cap", "stash_process",
          "grid_quant", "grid_sg_lds", "queue_block", "queue_static", "total_paths", "max_depth", "mode", "reserved")
W = {name: k for k, name in enumerate(FIELDS)}
# shape_flags
GRID, GRID_QUANT, SG, MATS16 = 1, 2, 4, 8
# setting_flags
MFMA, MATS_LDS, RAY_CACHE, STASH, TREE_LDS, FORCE_GLOBAL = 1, 2, 4, 8, 16, 32
DEFAULT_SETTINGS = MFMA | MATS_LDS | RAY_CACHE | STASH | TREE_LDS

N_RANDOM = 24000
SEED = 20260119

# both sides of: the 48 KiB table limit with (682) and without (2,048) materials in LDS, the 16-bit ids, and of the flat scan's
# 160 KiB image where the groups are the top level (n_levels == 1, top_cnt == "natural")
N_PADDED = (4, 8, 64, 256, 400, 680, 681, 682, 683, 684, 1000, 1500, 1800, 1900, 1960, 2000, 2044, 2047, 2048, 2049, 2052, 4096, 10004, 30000,
            65532, 65535, 65536)
N_PADDED_SMALL = (4, 8, 64, 256, 400, 484, 680, 681, 682, 683, 684)
TOTAL_PATHS = (0, 1, 64, 65, 10 ** 6, 2 ** 32 - 1)
MAX_DEPTH = (6, 65535, 65536)
GRIDS = ((1, 1), (64, 64), (240, 250))                      # 1, 4,096 and 60,000 cells
SHADOW = ((0, 0, 0, 0), (16, 16, 500, 3), (64, 64, 8000, 10), (128, 128, 60000, 64))  # off, small, medium, too large for LDS: nx, ny, entries, global


def base_case(**kw):
    """A cover-like scene under the default settings: flat scan, hit stash, 1024 threads, one block per CU."""
    c = dict(n_padded=484, n_levels=1, top_cnt=120, top_off=0, shape_flags=SG, grid_nu=0, grid_nv=0, sg_nx=32, sg_ny=32, sg_nentries=2000,
             sg_nglobal=4, n_lights=1, cu_count=256, blocks_per_cu=1, block_threads=1024, setting_flags=DEFAULT_SETTINGS, mats16=0, mats_l2=1,
             stash_cap=63, stash_process=63, grid_quant=0, grid_sg_lds=0, queue_block=0, queue_static=1, total_paths=10 ** 6, max_depth=50, mode=0,
             reserved=0)
    c.update(kw)
    return c


def pack(cases):
    out = np.zeros((len(cases), CASE_WORDS), dtype=np.uint32)
    for r, c in enumerate(cases):
        for name, v in c.items():
            out[r, W[name]] = v
    return out


def random_cases(n=N_RANDOM, seed=SEED):
    rs = np.random.RandomState(seed)

    def pick(seq, p=None):
        return seq[rs.choice(len(seq), p=p)]

    cases = []
    for _ in range(n):
        c = base_case()
        # half of the cases are small scenes (the ones whose tables fit LDS: most of the variants are theirs), a quarter of those
        # laid out for the cell grid
        small = rs.rand() < 0.5
        small_grid = small and rs.rand() < 0.25
        c["n_padded"] = pick(N_PADDED) if rs.rand() < 0.6 else 4 * int(rs.randint(1, 16385))
        if rs.rand() < 0.05:
            c["n_padded"] = int(rs.randint(4, 65537))
        if small:
            c["n_padded"] = pick(N_PADDED_SMALL)
        c["n_levels"] = 1 if small else pick((1, 2, 3), (0.4, 0.3, 0.3))
        natural = max(c["n_padded"] // 4 - 1, 1)
        c["top_cnt"] = pick((1, 32, 33, 128, natural), (0.15, 0.15, 0.15, 0.25, 0.3))
        c["top_off"] = 0 if c["n_levels"] == 1 else pick((c["n_padded"] // 4, 2000, 12000))
        flags = 0
        if small_grid or (not small and rs.rand() < 0.4):
            flags |= GRID
            c["grid_nu"], c["grid_nv"] = pick(GRIDS)
        if rs.rand() < 0.75:
            flags |= GRID_QUANT
        sg = pick(SHADOW, (0.2, 0.35, 0.25, 0.2))
        if sg[0]:
            flags |= SG
        c["sg_nx"], c["sg_ny"], c["sg_nentries"], c["sg_nglobal"] = sg
        if rs.rand() < 0.5:
            flags |= MATS16
        c["shape_flags"] = flags
        c["n_lights"] = pick((0, 1, 3), (0.2, 0.5, 0.3))
        c["cu_count"] = pick((256, 8))
        c["blocks_per_cu"] = pick((1, 2, 4), (0.5, 0.25, 0.25))
        c["block_threads"] = pick((256, 512, 1024), (0.2, 0.2, 0.6))
        s = 0
        for bit, p_on in ((MFMA, 0.8), (MATS_LDS, 0.7), (RAY_CACHE, 0.7), (STASH, 0.6), (TREE_LDS, 0.7), (FORCE_GLOBAL, 0.15)):
            if rs.rand() < p_on:
                s |= bit
        c["setting_flags"] = s
        c["mats16"] = pick((0, 1, 2))
        c["mats_l2"] = pick((1, 0), (0.7, 0.3))
        c["stash_cap"] = pick((63, 16, 15, 8), (0.55, 0.15, 0.15, 0.15))
        c["stash_process"] = pick((63, 0, 20))
        c["grid_quant"] = pick((0, 1))
        c["grid_sg_lds"] = pick((0, 1), (0.7, 0.3))
        c["queue_block"] = pick((0, 64, 200), (0.6, 0.2, 0.2))
        c["queue_static"] = pick((1, 0, 2), (0.6, 0.2, 0.2))
        c["total_paths"] = pick(TOTAL_PATHS)
        c["max_depth"] = pick(MAX_DEPTH, (0.45, 0.45, 0.1))
        c["mode"] = 1 if rs.rand() < (0.3 if small and not small_grid else 0.05) else 0
        cases.append(c)
    return cases


# ---- directed part: (base case, the field that is swept, the values).  Each sweep walks one field across the thresholds of the
# comparisons it takes part in, one entry (or one 16-byte step of the image) at a time around them.
def _around(*ts, step=1, reach=2):
    return sorted({t + k * step for t in ts for k in range(-reach, reach + 1) if t + k * step >= 0})


def _sweeps():
    B = base_case
    flat_nomats = B(setting_flags=DEFAULT_SETTINGS & ~MATS_LDS)
    valu = B(setting_flags=DEFAULT_SETTINGS & ~MFMA)
    tree = B(n_padded=20004, n_levels=3, top_cnt=79, top_off=6250)
    grid = B(n_padded=10004, shape_flags=SG | GRID | GRID_QUANT, grid_nu=64, grid_nv=64, sg_nx=128, sg_ny=128, sg_nentries=20000, sg_nglobal=2)
    grid_small = B(n_padded=400, shape_flags=SG | GRID, grid_nu=16, grid_nv=16)
    carry = B(mode=1)
    out = []
    # the table limit, the 16-bit ids
    for base in (B(), flat_nomats, valu, grid_small, carry, B(block_threads=256), B(setting_flags=DEFAULT_SETTINGS & ~STASH)):
        out.append((base, "n_padded", _around(682, 2048, 65535, reach=3)))
    # the filter's tiles (32 groups each, an even number of them), the largest top level, and the flat image's 160 KiB
    out.append((B(), "top_cnt", list(range(1, 164))))
    out.append((tree, "top_cnt", list(range(1, 164))))
    out.append((B(n_padded=2048, setting_flags=DEFAULT_SETTINGS & ~MATS_LDS), "top_cnt", list(range(380, 560))))
    # hierarchy in LDS or not
    out.append((tree, "top_off", list(range(0, 12000, 37)) + THRESHOLDS.get("tree.top_off", [])))
    # depth shares a register with the scan entry
    for base in (B(), tree, grid):
        out.append((base, "max_depth", [0, 1, 6, 65534, 65535, 65536, 65537, 2 ** 32 - 1]))
    # the queue: blocks of 128 or 256 paths, static part, shards
    for base in (B(), B(cu_count=8), B(block_threads=256, cu_count=8)):
        wpb = base["block_threads"] // 64
        t = 8192 * base["cu_count"] * wpb
        out.append((base, "total_paths", _around(0, 64, 128, 64 * wpb, 64 * wpb * base["cu_count"], 128 * wpb * base["cu_count"], t, 2 ** 32 - 3)))
        out.append((base, "queue_block", [0, 1, 63, 64, 65, 127, 128, 129, 4096]))
        out.append((base, "queue_static", [0, 1, 2, 3, 1000]))
    # the stash: capacity knob, processing threshold, blocks per CU
    for base in (B(), tree, grid, B(blocks_per_cu=2), B(n_padded=680)):
        out.append((base, "stash_cap", list(range(0, 66))))
        out.append((base, "stash_process", [0, 1, 15, 16, 43, 44, 45, 62, 63, 64]))
        out.append((base, "blocks_per_cu", [1, 2, 3, 4, 5, 8]))
        out.append((base, "block_threads", [64, 128, 256, 512, 960, 1024]))
        out.append((base, "n_lights", [0, 1, 2, 3]))
    # materials through L2: eight more records, at least sixteen; packed materials: at least 48
    for m16 in (0, 1, 2):
        for bpc in (1, 2):
            out.append((B(shape_flags=SG | MATS16, mats16=m16, blocks_per_cu=bpc), "n_padded", list(range(4, 700, 4))))
    # the found thresholds (recorded launcher, bisected): the image's byte budgets in the field that moves them
    for key, (base, field) in _THRESHOLD_BASES(B, flat_nomats, tree, grid, grid_small).items():
        vals = THRESHOLDS.get(key, [])
        if vals:
            out.append((base, field, vals))
    return out


def _THRESHOLD_BASES(B, flat_nomats, tree, grid, grid_small):
    return {
        "flat.sg_nentries": (B(), "sg_nentries"),
        "flat_bpc2.sg_nentries": (B(blocks_per_cu=2), "sg_nentries"),
        "flat_nomats.sg_nentries": (flat_nomats, "sg_nentries"),
        "flat_cache.sg_nentries": (B(setting_flags=DEFAULT_SETTINGS & ~STASH), "sg_nentries"),
        "carry.sg_nentries": (B(mode=1), "sg_nentries"),
        "grid_small.sg_nentries": (grid_small, "sg_nentries"),
        "grid_small.grid_nu": (dict(grid_small, grid_nv=64), "grid_nu"),
        "grid.grid_nu": (dict(grid, grid_nv=250), "grid_nu"),
        "grid_sg.sg_nentries": (dict(grid, grid_sg_lds=1), "sg_nentries"),
        "grid_sg_bpc2.sg_nentries": (dict(grid, grid_sg_lds=1, blocks_per_cu=2), "sg_nentries"),
        "grid_q.n_padded": (dict(grid, grid_quant=1), "n_padded"),
        "grid_q_bpc2.n_padded": (dict(grid, grid_quant=1, blocks_per_cu=2), "n_padded"),
        "grid_q_bpc4.n_padded": (dict(grid, grid_quant=1, blocks_per_cu=4), "n_padded"),
        "flat_cache_bpc4.n_padded": (B(setting_flags=DEFAULT_SETTINGS & ~STASH, blocks_per_cu=4), "n_padded"),
        "valu_cache_bpc4.n_padded": (B(setting_flags=DEFAULT_SETTINGS & ~MFMA, blocks_per_cu=4, block_threads=512), "n_padded"),
    }


# Where the recorded launcher's decisions change along each of the sweeps above (every change point, with its neighbours at the
# field's step: 8 entries of the shadow index are 16 bytes of image, as is one column of 8 cells' 16-bit starts)
THRESHOLDS = {'carry.sg_nentries': [6234, 6235, 6236, 6237],
 'flat.sg_nentries': [30810, 30811, 30812, 30813],
 'flat_bpc2.sg_nentries': [30810, 30811, 30812, 30813],
 'flat_cache.sg_nentries': [6234, 6235, 6236, 6237, 30810, 30811, 30812, 30813],
 'flat_cache_bpc4.n_padded': [681, 682, 683, 684],
 'flat_nomats.sg_nentries': [32698, 32699, 32700, 32701, 42426, 42427, 42428, 42429],
 'grid.grid_nu': [139, 140, 141, 142, 178, 179, 180, 181],
 'grid_q.n_padded': [99, 100, 101, 102, 15471, 15472, 15473, 15474],
 'grid_q_bpc2.n_padded': [99, 100, 101, 102, 15471, 15472, 15473, 15474],
 'grid_q_bpc4.n_padded': [99, 100, 101, 102, 15471, 15472, 15473, 15474],
 'grid_sg.sg_nentries': [9692, 9693, 9694, 9695],
 'grid_sg_bpc2.sg_nentries': [9692, 9693, 9694, 9695],
 'grid_small.grid_nu': [169, 170, 171, 172, 548, 549, 550, 551],
 'grid_small.sg_nentries': [16266, 16267, 16268, 16269, 25986, 25987, 25988, 25989],
 'tree.top_off': [4955, 4956, 4957, 4958, 6171, 6172, 6173, 6174, 8816, 8817, 8818, 8819],
 'valu_cache_bpc4.n_padded': [681, 682, 683, 684]}


def directed_cases():
    cases = []
    for base, field, values in _sweeps():
        for v in values:
            c = dict(base)
            c[field] = int(v)
            if field == "n_padded" and c["n_levels"] == 1 and not (c["shape_flags"] & GRID):
                c["top_cnt"] = min(max(c["n_padded"] // 4 - 1, 1), 128)  # a flat scene's top level is its groups
            cases.append(c)
    return cases


def all_cases():
    """(packed cases [n, 28] uint32, number of directed cases: they come first)"""
    d = directed_cases()
    return pack(d + random_cases()), len(d)


def digest(packed):
    return hashlib.sha256(np.ascontiguousarray(packed, dtype="<u4").tobytes()).hexdigest()


def row_hashes(words):
    """64-bit FNV-1a over the bytes of every row of a uint32 array."""
    b = np.ascontiguousarray(words, dtype="<u4").view(np.uint8).reshape(len(words), -1)
    h = np.full(len(words), 0xCBF29CE484222325, dtype=np.uint64)
    prime = np.uint64(0x100000001B3)
    with np.errstate(over="ignore"):
        for k in range(b.shape[1]):
            h = (h ^ b[:, k].astype(np.uint64)) * prime
    return h
