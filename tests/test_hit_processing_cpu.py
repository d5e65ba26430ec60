"""Hit processing over the material space, on the oracle alone (no GPU) -- and the seeded input generator that
tests/test_hit_processing.py feeds to the device.

material_records() is the material space: every type under both texture kinds, the smoothness, ior, tiling, luminance and colour
values at which hit processing changes behaviour.  incidences(oracle, record) is the incidence space for one record: random
incidences plus cases STEERED onto every comparison of Material::Scatter and DirectionalLight::Shade -- ndv > 0 and dn > 0 around
zero, XMVector3RefractV's k <= 0 at the critical angle, the coins prob > u and refl > u at equality, the diffuse basis choice
|n.x| < 0.5, the checker's (int)(tiling * u) at cell borders -- and the zero-length vectors of Shade.

The tests here keep the generator honest: (a) every branch is taken and every steered comparison is reached from both sides right
at equality, judged from the oracle's outputs; (b) few enough cases are masked (not scattered) or NaN that the device comparison
cannot hide a failure behind them; (c) away from the edges the oracle obeys the closed forms in binary64; (d) the reference's own
compiled Scatter gives the oracle's bits on the same inputs; (e) the material domain of include/rt_api.h is enforced by the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle.oracle_py import MATERIAL_DTYPE

F = np.float32
OPAQUE, METAL, GLASS, EMISSIVE = 0, 1, 2, 3
CONST, CHECKER = 0, 1
K255 = F(1.0) / F(255.0)
ULP1 = F(2.0 ** -23)            # one ulp of 1.0: the unit of "right at equality" for dot products of unit vectors
BELOW_ONE = F(1.0 - 2.0 ** -24)  # the largest uniform a draw can return

SMOOTHNESS = (0.0, 1.0, 8.0, 35.5, 64.0, 500.0, 2048.0)
IOR = (0.5, 1.0, 1.0 + 2.0 ** -23, 1.33, 1.5, 2.4, 10.0)
TILING = (1.0, 4.0, 2500.0, 1.0e6, -50.0, 2.0 ** 30)
LUMINANCE = (0.0, 8000.0, 1.0e6)
COLOURS = ((230, 128, 26), (51, 77, 26), (0, 0, 0), (255, 255, 255), (0, 255, 128), (255, 0, 1), (200, 120, 60), (13, 254, 97))

N_INCIDENCES = 4096
STOCK_VIEW = (12.0, 2.0, -2.5)
POS_AT_VIEW = (1.5, -2.25, 3.0)     # the hit position of the "view origin at the hit point" cases, and the second view origin
FAR_VIEW = (1.0e6, 2.0, -2.5)
POS_BELOW_VIEW = (8.0, 2.0, -2.5)   # STOCK_VIEW - (4, 0, 0): viewDir from the stock origin is (1, 0, 0) exactly
VIEW_ORIGINS = (STOCK_VIEW, POS_AT_VIEW, FAR_VIEW)


def _record(kind, tex=CONST, smoothness=0.0, ior=0.0, tiling=0.0, c0=0, c1=1, luminance=0.0):
    m = np.zeros(1, dtype=MATERIAL_DTYPE)
    m["type"], m["tex_type"] = kind, tex
    if kind != EMISSIVE:
        m["smoothness"] = smoothness
    if kind == GLASS:
        m["ior"] = ior
    else:
        m["rgb0"] = np.array(COLOURS[c0 % len(COLOURS)], F) * K255
        if tex == CHECKER:
            m["rgb1"] = np.array(COLOURS[c1 % len(COLOURS)], F) * K255
            m["tiling"] = tiling
    if kind == EMISSIVE:
        m["luminance"] = luminance
    return m


def material_records():
    """The material space: a list of one-element MATERIAL_DTYPE arrays, byte colours only.  Fields a type does not read stay 0."""
    out = []
    for kind in (OPAQUE, METAL):
        for i, s in enumerate(SMOOTHNESS):
            out.append(_record(kind, CONST, smoothness=s, c0=i + kind))
            out.append(_record(kind, CHECKER, smoothness=s, tiling=TILING[i % len(TILING)], c0=i + 2 + kind, c1=i + 3 + kind))
        out.append(_record(kind, CONST, smoothness=500.0, c0=2))  # black
        out.append(_record(kind, CONST, smoothness=1.0, c0=3))    # white
    for i, s in enumerate(SMOOTHNESS):
        out.append(_record(GLASS, smoothness=s, ior=IOR[i]))
        out.append(_record(GLASS, smoothness=s, ior=IOR[(i + 3) % len(IOR)]))
    for i, lum in enumerate(LUMINANCE):
        out.append(_record(EMISSIVE, CONST, luminance=lum, c0=i + 2))
    for i, t in enumerate(TILING):
        out.append(_record(EMISSIVE, CHECKER, tiling=t, luminance=LUMINANCE[i % len(LUMINANCE)], c0=i + 1, c1=i + 2))
    return out


def record_id(m):
    kind, tex = int(m["type"][0]), int(m["tex_type"][0])
    s = "%s-%s" % (("opaque", "metal", "glass", "emissive")[kind], ("const", "checker")[tex])
    if kind != EMISSIVE:
        s += "-s%g" % m["smoothness"][0]
    if kind == GLASS:
        s += "-ior%.9g" % m["ior"][0]
    if kind == EMISSIVE:
        s += "-lum%g" % m["luminance"][0]
    if tex == CHECKER:
        s += "-t%g" % m["tiling"][0]
    if kind != GLASS:
        s += "-c%d.%d.%d" % tuple(int(round(float(c) * 255.0)) for c in m["rgb0"][0])
    return s


def stock_sun(oracle):
    sun = oracle.RtLight()
    sdir = F(1.0) / np.sqrt(F(3.0))
    for k in range(3):
        sun.direction[k] = float(sdir)
        sun.color[k] = float(F((255, 247, 224)[k]) * K255)
    sun.luminance = 40000.0
    return sun


def suns(oracle):
    """The stock sun; one pointing against the +y normals of the axis-aligned cases; one with L = -viewDir for the hits at
    POS_BELOW_VIEW seen from the stock view origin; the stock sun scaled to length 0.51 and to 1.99 (unnormalised lights that the
    shadow index still takes for directions)."""
    out = [stock_sun(oracle)]
    for d in ((0.0, -1.0, 0.0), (-1.0, 0.0, 0.0)):
        l = stock_sun(oracle)
        for k in range(3):
            l.direction[k] = d[k]
        out.append(l)
    for scale in (0.51, 1.99):
        l = stock_sun(oracle)
        for k in range(3):
            l.direction[k] = float(F(l.direction[k]) * F(scale))
        out.append(l)
    return out


# ------------------------------------------------------------------ binary32 restatements (labels and steering only)
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def refract_k(rd, nrm, ior):
    """XMVector3RefractV's k as DielectricTransparent::Scatter reaches it, in binary32, and whether the ray leaves (dn > 0)"""
    dn = dot3(rd, nrm)
    inside = dn > 0
    eta = np.where(inside, F(ior), F(1.0) / F(ior)).astype(F)
    d = np.where(inside, dot3(rd, -nrm), dn).astype(F)
    k = F(1.0) - ((F(1.0) - d * d) * eta) * eta
    return k.astype(F), inside


def schlick(oracle, ndv):
    """DielectricOpaque's reflectance for a front-facing hit: f0 + (1 - f0) * pow(1 - sat(ndv), 5), pow through the oracle"""
    p = oracle.math_array(2, F(1.0) - np.clip(ndv, F(0), F(1)).astype(F), np.full(ndv.shape, 5.0, F))
    return (F(0.04) + (F(1.0) - F(0.04)) * p).astype(F)


def fresnel(oracle, rd, nrm, ior):
    """DielectricTransparent's reflection probability where it can refract: XMFresnelTerm(cosI, ior) through the oracle"""
    dn = dot3(rd, nrm)
    cos_i = np.where(dn > 0, dn, dot3(rd, -nrm)).astype(F)
    L = oracle.lib()
    return np.array([L.orc_fresnel_term(float(c), float(ior)) for c in cos_i], F)


def uv_of(nrm):
    """Sphere::ComputeUV as the device restates it: 0.5 n.x + 0.5, 0.5 n.z + 0.5"""
    return np.stack([F(0.5) * nrm[:, 0] + F(0.5), F(0.5) * nrm[:, 2] + F(0.5)], 1).astype(F)


# ------------------------------------------------------------------ the incidence generator
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _tangent(rng, nrm):
    t = np.cross(nrm, rng.normal(size=nrm.shape))
    return t / np.linalg.norm(t, axis=1, keepdims=True)


def _at_cosine(rng, nrm, cosv):
    """unit directions with d . n = -cosv (cosv > 0 faces the ray)"""
    cosv = np.asarray(cosv, np.float64)
    return -cosv[:, None] * nrm + np.sqrt(np.maximum(0.0, 1.0 - cosv ** 2))[:, None] * _tangent(rng, nrm)


def _random_block(rng, n, kind, facing=0.75):
    """random unit normals and directions; about `facing` of the hits on an opaque or metal record face the ray (half on others)"""
    nrm = _unit(rng, n)
    rd = _unit(rng, n)
    front = np.einsum("ij,ij->i", rd, nrm) < 0
    want_front = rng.random(n) < (facing if kind in (OPAQUE, METAL) else 0.5)
    rd[front != want_front] *= -1.0
    draws = rng.uniform(0, 1, (n, 3))
    draws[: n // 3, 0] *= 0.05  # the mirror side of the coin, often
    return rd, nrm, draws


def _facing_block(rng, n, lo=0.05, hi=1.0):
    nrm = _unit(rng, n)
    return _at_cosine(rng, nrm, rng.uniform(lo, hi, n)), nrm


def _with_nx(rng, nx):
    """unit normals (binary64) whose x component is nx"""
    a = rng.uniform(0, 2 * np.pi, len(nx))
    s = np.sqrt(np.maximum(0.0, 1.0 - np.asarray(nx, np.float64) ** 2))
    return np.stack([np.asarray(nx, np.float64), s * np.cos(a), s * np.sin(a)], 1)


def _ulps(x, j):
    """x moved by j binary32 ulps towards +inf (j < 0: towards -inf), |j| <= 8"""
    x = np.asarray(x, F).copy()
    j = np.broadcast_to(np.asarray(j, np.int64), x.shape)
    for step in range(1, 9):
        x = np.where(j >= step, np.nextafter(x, F(np.inf)), np.where(j <= -step, np.nextafter(x, F(-np.inf)), x)).astype(F)
    return x


def _checker_normals(rng, n, tiling):
    """unit normals whose tiling * u (first half) or tiling * v lies within 2 ulp of an integer: the component c with
    0.5 c + 0.5 nearest m / tiling, moved by -2 .. 2 ulps"""
    t = float(tiling)
    span = min(abs(t), 2.0 ** 24)
    m = np.rint(rng.uniform(0.02, 0.98, n) * span) * np.sign(t) * (abs(t) / span)
    m[:2] = (0.0, t)  # the uv corners 0 and 1
    c = _ulps(np.clip(2.0 * (m / t) - 1.0, -1.0, 1.0).astype(F) + F(0), rng.integers(-2, 3, n))
    c = np.clip(c, F(-1), F(1))
    nrm = _with_nx(rng, c)
    nrm[n // 2:] = nrm[n // 2:, ::-1]  # the z component for the second half
    out = nrm.astype(F)
    out[: n // 2, 0] = c[: n // 2]
    out[n // 2:, 2] = c[n // 2:]
    return out


# The blocks of incidences(), in order, with their sizes; what is left of the 4,096 is random.  The one place that says where a
# block's rows are: incidences() checks its running total against it after every block, the tests ask block_rows().
BLOCKS = (("facing edges", 384), ("critical angle", 272), ("coin draws", 320), ("diffuse mapping", 160), ("basis choice", 128),
          ("checker borders", 128), ("not unit vectors", 128), ("zero-length vectors", 96))
COIN_REPEATS = 5  # the coin block is the same 64 incidences five times: u = coin, coin - 1 ulp, coin + 1 ulp, 0, the largest uniform


def block_rows(name, part=None):
    """the rows of a block of incidences() as a slice; part k of the coin block: its k-th repeat of the 64 incidences"""
    at = 0
    for b, size in BLOCKS:
        if b == name:
            if part is None:
                return slice(at, at + size)
            step = size // COIN_REPEATS
            return slice(at + part * step, at + (part + 1) * step)
        at += size
    raise KeyError(name)


def incidences(oracle, record, n=N_INCIDENCES, seed=0):
    """[n, 12] binary32 inputs of rt_unit_scatter for one record: ray direction, hit position, hit normal, three uniforms.  The
    coin values of the steered draws come from the oracle (orc_fresnel_term, math_array op 2)."""
    assert n == N_INCIDENCES
    kind, tex = int(record["type"][0]), int(record["tex_type"][0])
    ior, tiling = float(record["ior"][0]), float(record["tiling"][0])
    rng = np.random.default_rng([20250117, seed, kind, tex, int(record["smoothness"].view(np.uint32)[0]), int(record["ior"].view(np.uint32)[0]),
                                 int(record["tiling"].view(np.uint32)[0])])
    blocks = []

    def add(rd, nrm, draws=None, pos=None):
        m = len(rd)
        rd, nrm = np.asarray(rd, F), np.asarray(nrm, F)
        draws = rng.uniform(0, 1, (m, 3)) if draws is None else draws
        pos = rng.uniform(-5, 5, (m, 3)) if pos is None else pos
        blocks.append(np.concatenate([rd, np.asarray(pos, F), nrm, np.asarray(draws, F)], 1).astype(F))

    def filler(m):
        add(*_random_block(rng, m, kind))

    def done(name):
        assert sum(len(b) for b in blocks) == block_rows(name).stop, name

    # --- facing edges (384)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    pairs = np.array([(a, b) for a in range(6) for b in range(6) if a % 3 != b % 3])  # 24 pairs with n . d == 0 exactly
    pairs = pairs[np.arange(96) % 24]
    add(axes[pairs[:, 1]], axes[pairs[:, 0]])
    nrm = _unit(rng, 192)
    add(_at_cosine(rng, nrm, np.where(np.arange(192) % 2 == 0, 1.0, -1.0) * 10.0 ** rng.uniform(-8, -3, 192)), nrm)
    nrm = _unit(rng, 96).astype(F)
    add(np.where((np.arange(96) % 4 != 3)[:, None], -nrm, nrm), nrm)  # d = -n (three in four) and d = +n, exactly
    done("facing edges")
    # --- the critical angle (272): sine = (1 / eta) (1 + k 2^-23), |k| <= 8, on the side where eta > 1
    if kind == GLASS and ior != 1.0:
        eta = ior if ior > 1.0 else 1.0 / ior
        kk = (np.arange(272) % 17 - 8).astype(np.float64)
        sine = np.minimum(1.0, (1.0 / eta) * (1.0 + kk * 2.0 ** -23))
        nrm = _unit(rng, 272)
        cosv = np.sqrt(1.0 - sine ** 2) * (-1.0 if ior > 1.0 else 1.0)  # ior > 1: from inside (d . n > 0)
        add(_at_cosine(rng, nrm, cosv), nrm)
    else:
        filler(272)
    done("critical angle")
    # --- coin draws (320): u = the oracle's coin value, one ulp either side, 0 and the largest uniform
    if kind in (OPAQUE, GLASS):
        if kind == OPAQUE:
            rd, nrm = _facing_block(rng, 64, 0.0, 1.0)
            rd, nrm = rd.astype(F), nrm.astype(F)
            coin = schlick(oracle, dot3(-rd, nrm))
        else:
            rd, nrm, _ = _random_block(rng, 64, kind)
            rd, nrm = rd.astype(F), nrm.astype(F)
            coin = fresnel(oracle, rd, nrm, ior)
        coin = np.where(np.isfinite(coin), coin, F(0.5)).astype(F)
        for u in (coin, np.nextafter(coin, F(-np.inf)), np.nextafter(coin, F(np.inf)), np.zeros(64, F), np.full(64, BELOW_ONE)):
            draws = rng.uniform(0, 1, (64, 3))
            draws[:, 0] = u
            add(rd, nrm, draws)
    else:
        filler(320)
    done("coin draws")
    # --- diffuse mapping (160): the corners of the hemisphere map
    if kind == OPAQUE:
        rd, nrm = _facing_block(rng, 160, 0.2, 1.0)
        draws = np.zeros((160, 3))
        draws[:, 0] = BELOW_ONE
        draws[:, 1] = np.array([0.0, BELOW_ONE])[np.arange(160) % 2]
        draws[:, 2] = np.array([0.0, 0.25, 0.5, 0.75, BELOW_ONE])[(np.arange(160) // 2) % 5]
        add(rd, nrm, draws)
    else:
        filler(160)
    done("diffuse mapping")
    # --- basis choice (128): |n.x| within 2 ulp of 0.5, on the diffuse side of the coin
    nx = _ulps(np.full(128, 0.5, F), np.arange(128) % 5 - 2) * np.where((np.arange(128) // 5) % 2 == 0, F(1), F(-1))
    nrm = _with_nx(rng, nx)
    rd = _at_cosine(rng, nrm, rng.uniform(0.2, 1.0, 128))
    nrm = nrm.astype(F)
    nrm[:, 0] = nx
    draws = rng.uniform(0, 1, (128, 3))
    draws[:, 0] = BELOW_ONE
    add(rd, nrm, draws)
    done("basis choice")
    # --- checker borders (128)
    if tex == CHECKER and kind != GLASS:
        nrm = _checker_normals(rng, 128, tiling)
        add(_at_cosine(rng, nrm.astype(np.float64), rng.uniform(0.1, 1.0, 128)), nrm)
    else:
        filler(128)
    done("checker borders")
    # --- vectors that are not unit vectors (128): normals of length 1 +- 4 ulp, negated normals (a hollow sphere's inner
    # surface), ray directions of length 0.5 and 2
    rd, nrm = _facing_block(rng, 128, 0.05, 1.0)
    rd, nrm = rd.astype(F), nrm.astype(F)
    nrm[:32] = nrm[:32] * (F(1.0) + F(4.0) * ULP1 * np.where(np.arange(32) % 2 == 0, F(1), F(-1)))[:, None]
    nrm[32:64] = -nrm[32:64]
    rd[64:96] = rd[64:96] * F(0.5)
    rd[96:128] = rd[96:128] * F(2.0)
    add(rd, nrm)
    done("not unit vectors")
    # --- the zero-length vectors of Shade (96): hits AT a view origin (viewDir = 0), and hits whose viewDir from the stock view
    # origin is (1, 0, 0) exactly -- the third sun is (-1, 0, 0), so L + viewDir = 0
    rd, nrm, draws = _random_block(rng, 96, kind)
    pos = np.where((np.arange(96) < 48)[:, None], np.array(POS_AT_VIEW), np.array(POS_BELOW_VIEW))
    add(rd, nrm, draws, pos)
    done("zero-length vectors")
    # --- random incidences: the rest
    filler(n - sum(len(b) for b in blocks))
    out = np.concatenate(blocks).astype(F)
    assert out.shape == (n, 12)
    return out


def in17_of(inc):
    """the oracle's 17-float form of the 12-float device input: ray origin (pos - d), direction, pos, normal, uv, uniforms"""
    rd, pos, nrm, draws = inc[:, 0:3], inc[:, 3:6], inc[:, 6:9], inc[:, 9:12]
    return np.concatenate([pos - rd, rd, pos, nrm, uv_of(nrm), draws], 1).astype(F)


def hits8_of(inc):
    return np.concatenate([inc[:, 3:6], inc[:, 6:9], uv_of(inc[:, 6:9])], 1).astype(F)


def oracle_scatter11(oracle, record, inc):
    """the oracle's answer in rt_unit_scatter's layout WITHOUT the last three columns' light: flag, attenuation, direction, draws"""
    o = oracle.scatter_n(record, in17_of(inc))
    out = np.concatenate([o[:, 0:4], o[:, 7:10], o[:, 10:11]], 1)
    if int(record["type"][0]) == EMISSIVE:
        out[:, 1:4] = 1.0  # Emissive::Scatter leaves outAttenuation untouched; the device reports 1
    return out


def oracle_case_table(oracle, record, inc):
    """[n, 8 + 3 * views * suns]: scatter's 8 columns, then Emit + Shade for every (view origin, sun), view-major"""
    cols = [oracle_scatter11(oracle, record, inc)]
    h8 = hits8_of(inc)
    for vo in VIEW_ORIGINS:
        for sun in suns(oracle):
            cols.append(oracle.emit_shade_n(record, sun, vo, h8))
    return np.concatenate(cols, 1)


@pytest.fixture(scope="module")
def generated(oracle):
    """every record with its incidences and the oracle's answers, computed once for the module"""
    oracle.lib().orc_set_sampler(0)
    out = []
    for r, m in enumerate(material_records()):
        inc = incidences(oracle, m)
        out.append((m, inc, oracle_case_table(oracle, m, inc)))
    return out


# ------------------------------------------------------------------ (a) coverage
def _mirror64(rd, nrm):
    rd, nrm = rd.astype(np.float64), nrm.astype(np.float64)
    r = rd - 2.0 * np.einsum("ij,ij->i", rd, nrm)[:, None] * nrm
    return r / np.maximum(np.linalg.norm(r, axis=1, keepdims=True), 1e-300)


def branch_labels(record, inc, table):
    """the branch each case took, from the oracle's outputs (flag, draws consumed, direction against the mirror direction)"""
    kind = int(record["type"][0])
    rd, nrm = inc[:, 0:3], inc[:, 6:9]
    flag, used, d = table[:, 0] == 1, table[:, 7], table[:, 4:7].astype(np.float64)
    with np.errstate(invalid="ignore"):
        is_mirror = np.abs(d - _mirror64(rd, nrm)).max(axis=1) < 1e-4
    lab = np.full(len(inc), "", dtype=object)
    if kind == OPAQUE:
        lab[~flag] = "opaque back-facing"
        lab[flag & (used == 1)] = "opaque mirror"
        lab[flag & (used == 3)] = "opaque diffuse"
    elif kind == METAL:
        lab[~flag] = "metal back-facing"
        lab[flag] = "metal scatter"
    elif kind == GLASS:
        k, inside = refract_k(rd, nrm, float(record["ior"][0]))
        lab[:] = "glass reflecting although it could refract"
        lab[~is_mirror & ~inside] = "glass refracting on the way in"
        lab[~is_mirror & inside] = "glass refracting on the way out"
        lab[is_mirror & (k <= 0)] = "total internal reflection"
    else:
        lab[:] = "emissive"
    return lab


BRANCHES = ("opaque mirror", "opaque diffuse", "opaque back-facing", "metal scatter", "metal back-facing",
            "glass reflecting although it could refract", "glass refracting on the way in", "glass refracting on the way out",
            "total internal reflection", "emissive")


def test_every_branch_and_both_sides_of_every_steered_comparison_are_reached(oracle, generated):
    """(a) Over the full generated set every branch of Material::Scatter is taken by >= 200 cases, and both sides of every steered
    comparison are reached RIGHT AT equality by >= 20 cases each.  The side a case took is read from the oracle's outputs (flag,
    draws consumed, scattered direction); how near it was comes from the inputs: for the coins the uniform IS the oracle's coin
    value or its binary32 neighbour; for ndv, dn and k, sums of products of unit-length operands, "1 ulp" is one ulp of 1.0
    (2^-23); for |n.x| it is one ulp of 0.5."""
    counts = dict.fromkeys(BRANCHES, 0)
    sides = {}

    def side(name, truth, n):
        key = "%s %s" % (name, "true" if truth else "false")
        sides[key] = sides.get(key, 0) + int(n)

    for m, inc, table in generated:
        kind = int(m["type"][0])
        lab = branch_labels(m, inc, table)
        assert (lab != "").all()
        for b in BRANCHES:
            counts[b] += int((lab == b).sum())
        rd, nrm, u0 = inc[:, 0:3], inc[:, 6:9], inc[:, 9]
        flag, used = table[:, 0] == 1, table[:, 7]
        if kind in (OPAQUE, METAL):
            ndv = dot3(-rd, nrm)
            near = np.abs(ndv) <= ULP1
            side("ndv > 0", True, (near & flag).sum())
            side("ndv > 0", False, (near & ~flag).sum())
            assert ((ndv > 0) == flag).all()  # the binary32 restatement of the dot product labels every case as the oracle does
        if kind == OPAQUE:
            front = flag & (dot3(-rd, nrm) > 0)
            coin = np.zeros(len(inc), F)
            coin[front] = schlick(oracle, dot3(-rd, nrm)[front])
            mirror = front & (used == 1)
            side("refl > u", True, (mirror & (u0 == np.nextafter(coin, F(-np.inf)))).sum())
            side("refl > u", False, (front & ~mirror & (u0 == coin)).sum())
            diffuse = front & (used == 3)
            ax = np.abs(nrm[:, 0])
            side("|n.x| < 0.5", True, (diffuse & (ax == np.nextafter(F(0.5), F(0)))).sum())
            side("|n.x| < 0.5", False, (diffuse & (ax == F(0.5))).sum())
        if kind == GLASS:
            ior = float(m["ior"][0])
            k, inside = refract_k(rd, nrm, ior)
            dn = dot3(rd, nrm)
            near = np.abs(dn) <= ULP1
            side("dn > 0", True, (near & (dn > 0)).sum())
            side("dn > 0", False, (near & ~(dn > 0)).sum())
            tir = lab == "total internal reflection"
            neark = np.abs(k) <= ULP1
            side("k <= 0", True, (neark & tir).sum())
            side("k <= 0", False, (neark & (k > 0)).sum())
            # with u = the largest uniform only a hit that cannot refract still reflects: the oracle's k <= 0 is the restated one
            top = u0 == BELOW_ONE
            assert ((lab[top] == "total internal reflection") == (k[top] <= 0)).all()
            can = k > 0
            coin = np.zeros(len(inc), F)
            steered = block_rows("coin draws")
            coin[steered] = fresnel(oracle, rd[steered], nrm[steered], ior)
            st = np.zeros(len(inc), bool)
            st[steered] = True
            refl = lab == "glass reflecting although it could refract"
            side("prob > u", True, (st & can & refl & (u0 == np.nextafter(coin, F(-np.inf)))).sum())
            side("prob > u", False, (st & can & ~refl & (u0 == coin)).sum())
    print("branch counts:", counts)
    print("sides reached at equality:", sides)
    for b in BRANCHES:
        assert counts[b] >= 200, (b, counts[b])
    for name in ("ndv > 0", "dn > 0", "k <= 0", "prob > u", "refl > u", "|n.x| < 0.5"):
        for truth in ("true", "false"):
            assert sides.get("%s %s" % (name, truth), 0) >= 20, (name, truth, sides)


# ------------------------------------------------------------------ (b) caps
MAX_UNSCATTERED = 0.30  # per record of type 0 or 1
MAX_NAN = 0.01          # of all cases


def unscattered_fraction(table):
    return float((table[:, 0] == 0).mean())


def nan_case_fraction(tables):
    """share of (case, view origin, sun) combinations with a NaN anywhere in the 11 outputs rt_unit_scatter would report"""
    bad = total = 0
    for t in tables:
        head = np.isnan(t[:, :8]).any(axis=1)
        tail = np.isnan(t[:, 8:]).reshape(len(t), -1, 3).any(axis=2)
        bad += int((head[:, None] | tail).sum())
        total += tail.size
    return bad / float(total)


def test_caps_on_masked_and_nan_cases(generated):
    """(b) Conditions on the generator, not measurements: the device comparison masks the attenuation and direction of hits that do
    not scatter and compares a NaN only by position, so neither may be common."""
    worst = 0.0
    for m, inc, table in generated:
        if int(m["type"][0]) in (OPAQUE, METAL):
            f = unscattered_fraction(table)
            worst = max(worst, f)
            assert f <= MAX_UNSCATTERED, (record_id(m), f)
    nan = nan_case_fraction([t for _, _, t in generated])
    print("largest share of unscattered cases of an opaque or metal record: %.4f; NaN share of all cases: %.6f" % (worst, nan))
    assert nan <= MAX_NAN


# ------------------------------------------------------------------ (c) closed forms in binary64
def test_oracle_obeys_the_closed_forms_away_from_the_edges(oracle, generated):
    """(c) Mirror direction, Snell's law, the Schlick and Fresnel coin values and the Blinn-Phong value in binary64, for the cases
    with unit vectors away from the edges.  Bounds, with eps = 2^-24 (binary32 unit roundoff):
      mirror: reflect is one dot product (3 products, 2 sums), a doubling, 3 fused-free multiply-subtracts on components <= 3 in
        magnitude, then normalize (dot, sqrt, divide): <= ~16 roundings of values <= 3, and the inputs' own departure from unit
        length (<= 3 eps each) enters the binary64 form identically.  Bound 64 eps on each component of the unit result.
      Snell: refract adds k's chain (6 roundings, amplified by 1 / (2 sqrt k)) -- restricted to k >= 0.01, amplification <= 5 -- and
        a reciprocal of ior rounded once (relative eps, times eta <= 10 -> the sine): bound 512 eps on |sin_t - eta sin_i|.
      Schlick: 1 - ndv (ndv carries <= 4 eps), pow of rt_powf (<= 2 ulp claimed by the math tests), one multiply, one add: for
        x = 1 - ndv in [0, 1], d(x^5) = 5 x^4 dx <= 20 eps; bound 32 eps absolute.  Read off the coin: u = coin - 1 ulp reflects,
        u = coin does not.
      Blinn-Phong: relative bound.  nDotH carries <= 8 eps absolute, so pow(nDotH, s) carries s * 8 eps / nDotH relative: cases
        with nDotH >= 0.5 and s <= 64 -> <= 1024 eps.  x = 1 - nDotV carries <= 8 eps absolute, so x^5 -- all of the reflectance
        of a black metal -- carries 5 * 8 eps / x relative: cases with x >= 0.1 -> <= 400 eps.  The other ~12 operations add
        <= 16 eps: bound 2048 eps relative, applied where radiance > 0."""
    eps = 2.0 ** -24
    n_mirror = n_snell = n_schlick = n_fresnel = n_bp = 0
    sun = suns(oracle)[0]
    L = np.array(list(sun.direction), np.float64)
    rad = np.array(list(sun.color), np.float64) * float(sun.luminance)
    for m, inc, table in generated:
        kind = int(m["type"][0])
        rd, pos, nrm, u0 = inc[:, 0:3].astype(np.float64), inc[:, 3:6].astype(np.float64), inc[:, 6:9].astype(np.float64), inc[:, 9]
        unit = (np.abs(np.linalg.norm(rd, axis=1) - 1) < 1e-6) & (np.abs(np.linalg.norm(nrm, axis=1) - 1) < 1e-6)
        lab = branch_labels(m, inc, table)
        d = table[:, 4:7].astype(np.float64)
        dn = np.einsum("ij,ij->i", rd, nrm)
        # mirror
        sel = unit & np.isin(lab, ["opaque mirror", "metal scatter", "glass reflecting although it could refract", "total internal reflection"])
        assert np.abs(d[sel] - _mirror64(rd, nrm)[sel]).max(initial=0.0) <= 64 * eps
        n_mirror += int(sel.sum())
        if kind == GLASS:
            ior = float(F(m["ior"][0]))
            eta = np.where(dn > 0, ior, 1.0 / ior)
            k64 = 1.0 - eta * eta * (1.0 - dn * dn)
            sel = unit & np.isin(lab, ["glass refracting on the way in", "glass refracting on the way out"]) & (k64 >= 0.01)
            n_out = np.where(dn > 0, -1.0, 1.0)[:, None] * nrm
            sin_i = np.linalg.norm(rd - np.einsum("ij,ij->i", rd, n_out)[:, None] * n_out, axis=1)
            sin_t = np.linalg.norm(d - np.einsum("ij,ij->i", d, n_out)[:, None] * n_out, axis=1)
            assert np.abs(sin_t - eta * sin_i)[sel].max(initial=0.0) <= 512 * eps
            assert (np.einsum("ij,ij->i", d, n_out)[sel] < 0).all()  # the refracted ray goes through
            n_snell += int(sel.sum())
            # Fresnel (XMFresnelTerm's closed form: unpolarised dielectric reflectance with g^2 = ior^2 + c^2 - 1), read off the
            # steered coins.  25 operations, two divisions by (g + c)^2 and (c (g - c) + 1)^2, both >= 0.25 for c >= 0.1 and
            # g^2 >= 0.01 on these records: bound 1024 eps absolute on a value in [0, 1].
            st = np.zeros(len(inc), bool)
            st[block_rows("coin draws", 0)] = True  # the repeat with u = coin exactly
            c = np.abs(dn)
            g2 = ior * ior + c * c - 1.0
            sel = st & unit & (c >= 0.1) & (g2 >= 0.01) & (k64 >= 0.01)
            g = np.sqrt(np.abs(g2))
            with np.errstate(all="ignore"):
                fr = 0.5 * ((g - c) / (g + c)) ** 2 * (1.0 + ((c * (g + c) - 1.0) / (c * (g - c) + 1.0)) ** 2)
            assert np.abs(u0.astype(np.float64) - fr)[sel].max(initial=0.0) <= 1024 * eps
            n_fresnel += int(sel.sum())
        if kind == OPAQUE:
            st = np.zeros(len(inc), bool)
            st[block_rows("coin draws", 0)] = True
            sel = st & unit & (-dn > 0)
            sch = 0.04 + 0.96 * (1.0 - np.clip(-dn, 0, 1)) ** 5
            assert np.abs(u0.astype(np.float64) - sch)[sel].max(initial=0.0) <= 32 * eps
            n_schlick += int(sel.sum())
        if kind in (OPAQUE, METAL, GLASS):
            s = float(m["smoothness"][0])
            vd = np.array(STOCK_VIEW)[None, :] - pos
            vlen = np.linalg.norm(vd, axis=1)
            with np.errstate(all="ignore"):
                vd = vd / vlen[:, None]
                h = L[None, :] + vd
                h = h / np.linalg.norm(h, axis=1, keepdims=True)
                ndl = np.clip(nrm @ L, 0, 1)
                ndh = np.clip(np.einsum("ij,ij->i", nrm, h), 0, 1)
                ndvv = np.clip(np.einsum("ij,ij->i", vd, nrm), 0, 1)
                uv = uv_of(inc[:, 6:9]).astype(np.float64)
                t = float(m["tiling"][0])
                odd = ((np.trunc(t * uv[:, 0]) % 2) != (np.trunc(t * uv[:, 1]) % 2)) if int(m["tex_type"][0]) == CHECKER else np.zeros(len(inc), bool)
                tex = np.where(odd[:, None], m["rgb1"][0].astype(np.float64), m["rgb0"][0].astype(np.float64))
                albedo = tex if kind == OPAQUE else np.zeros_like(tex)
                f0 = tex if kind == METAL else np.full_like(tex, float(F(0.04)))
                refl = f0 + (1.0 - f0) * ((1.0 - ndvv) ** 5)[:, None]
                want = (rad[None, :] * ndl[:, None]) * (albedo + refl * 0.125 * (s + 8.0) * (ndh ** s)[:, None])
            got = table[:, 8:11].astype(np.float64)  # stock view, stock sun
            # away from the edges: a unit normal, a real view direction, nDotH well inside, no checker border in the way
            cellu, cellv = t * uv[:, 0], t * uv[:, 1]
            border = (np.abs(cellu - np.rint(cellu)) < 1e-3 * max(1.0, abs(t))) | (np.abs(cellv - np.rint(cellv)) < 1e-3 * max(1.0, abs(t)))
            sel = unit & (vlen > 1e-3) & (ndh >= 0.5) & (1.0 - ndvv >= 0.1) & (ndl > 1e-3) & (s <= 64) & ~(border & (int(m["tex_type"][0]) == CHECKER))
            ok = np.abs(got - want)[sel] <= 2048 * eps * np.abs(want)[sel] + 1e-30
            assert ok.all(), (record_id(m), int((~ok).sum()))
            n_bp += int(sel.sum())
    print("closed forms checked: mirror %d, Snell %d, Schlick %d, Fresnel %d, Blinn-Phong %d cases" % (n_mirror, n_snell, n_schlick, n_fresnel, n_bp))
    assert min(n_mirror, n_snell, n_schlick, n_fresnel, n_bp) >= 200


# ------------------------------------------------------------------ (d) the reference's compiled Scatter
def test_reference_scatter_gives_the_oracles_bits_on_the_generated_inputs(oracle, generated):
    """(d) Where oracle/_ref/libref.so exists: the reference's own Scatter, compiled from its sources, on the generated inputs, by
    the rule of tests/test_reference_code_cpu.py -- the reference draws from its per-material Halton counters, so the oracle runs in
    reference-counter mode on the same hits in the same order; flag, attenuation and origin equal bit for bit, and a direction may
    differ only where a diffuse bounce's hemisphere sample differs through libm's cos/sin, which the rule then explains.
    What this reaches: the reference draws its own uniforms, so the STEERED uniforms of the generated inputs (the coin values
    +- 1 ulp, the corners of the hemisphere map) are ignored here -- no entry of the reference's code takes a uniform from outside.
    The reference's Scatter sees the geometric edges only: n . d = 0, grazing, d = -+n, the critical angle, |n.x| at 0.5, checker
    borders, vectors that are not unit vectors.  The steered uniforms are checked against the oracle's own coin values in (a) and
    against the closed forms in (c)."""
    import test_reference_code_cpu as T
    from oracle import ref_py
    if not os.path.exists(ref_py.LIB_PATH) and not ref_py.reference_present():
        pytest.skip("neither oracle/_ref/libref.so nor the reference's sources exist on this machine")
    ref_py.lib()
    L = oracle.lib()
    L.orc_use_reference_halton_counters(1)
    try:
        excused = rows = 0
        for m, inc, _ in generated:
            in17 = in17_of(inc)
            mat = ref_py.Material(m)
            r_out, cnt = mat.scatter(in17[:, :14])
            mat.close()
            o_out = oracle.scatter_n(m, in17, use_counters=True)
            label = record_id(m)
            T.assert_same(r_out[:, :7], o_out[:, :7], label + ": flag, attenuation, origin")
            excused += T.explain_diffuse(ref_py, oracle, cnt, in17[:, 9:12], r_out[:, 7:10], o_out[:, 7:10], label)
            rows += len(inc)
        print("reference Scatter: %d hits, %d diffuse directions differ through libm, all explained" % (rows, excused))
        assert excused <= 0.05 * rows
    finally:
        L.orc_use_reference_halton_counters(0)


# ------------------------------------------------------------------ (e) the material domain
def offenders():
    """(what, record) pairs, one per clause of the material domain (include/rt_api.h at rt_material)"""
    nan, inf = float("nan"), float("inf")
    out = []

    def bad(field, base, **kw):
        m = base.copy()
        for k, v in kw.items():
            m[k] = v
        out.append((field, m))

    opaque_checker = _record(OPAQUE, CHECKER, smoothness=16.0, tiling=4.0)
    bad("type", _record(OPAQUE, smoothness=16.0), type=4)
    bad("type", _record(OPAQUE, smoothness=16.0), type=0xffffffff)
    bad("tex_type", _record(METAL, smoothness=1.0), tex_type=2)
    bad("smoothness", _record(OPAQUE), smoothness=nan)
    bad("smoothness", _record(METAL), smoothness=inf)
    bad("smoothness", _record(GLASS, ior=1.5), smoothness=-inf)
    bad("ior", _record(GLASS, smoothness=16.0), ior=nan)
    bad("luminance", _record(EMISSIVE), luminance=inf)
    bad("rgb0", _record(OPAQUE, smoothness=16.0), rgb0=np.array([0.5, nan, 0.5], F))
    bad("rgb0", _record(EMISSIVE, luminance=1.0), rgb0=np.array([inf, 0.5, 0.5], F))
    bad("rgb1", opaque_checker, rgb1=np.array([0.5, 0.5, nan], F))
    bad("tiling", opaque_checker, tiling=nan)
    bad("tiling", opaque_checker, tiling=inf)
    bad("tiling", opaque_checker, tiling=float(np.nextafter(F(2.0 ** 30), F(np.inf))))  # the product leaves int
    bad("tiling", _record(EMISSIVE, CHECKER, tiling=4.0, luminance=1.0), tiling=-3.0e9)
    bad("tiling", _record(METAL, CHECKER, smoothness=1.0, tiling=4.0), tiling=4.0e9)
    return out


def unread_nan_records():
    """records with NaN in every field their type does not read: inside the domain"""
    nan = float("nan")
    out = []
    m = _record(OPAQUE, CONST, smoothness=16.0)
    m["ior"], m["tiling"], m["rgb1"], m["luminance"] = nan, nan, nan, nan
    out.append(m)
    m = _record(METAL, CHECKER, smoothness=1.0, tiling=4.0)
    m["ior"], m["luminance"] = nan, nan
    out.append(m)
    m = _record(GLASS, smoothness=16.0, ior=1.5)
    m["tiling"], m["rgb0"], m["rgb1"], m["luminance"] = 3.0e9, nan, nan, nan
    out.append(m)
    m = _record(EMISSIVE, CONST, luminance=100.0)
    m["smoothness"], m["ior"], m["tiling"], m["rgb1"] = nan, nan, float("inf"), nan
    out.append(m)
    return out


def domain_scene(oracle, record=None, at=2, sky=None):
    """the three-sphere stock scene with `record` as sphere `at`'s material and `sky` as the sky's"""
    sc = oracle.build_scene("three", 1, 2.0)
    if record is not None:
        sc.materials[at] = record[0]
    if sky is not None:
        sc.sky = oracle.RtMaterial.from_buffer_copy(sky.tobytes())
    return sc


def test_oracle_refuses_records_outside_the_material_domain(oracle):
    """(e) orc_scene_upload and the single-material unit entries refuse one offender per clause of the domain, naming the sphere (or
    the sky) and the field; a NaN in a field the record's type does not read is accepted."""
    inc = np.zeros((4, 12), F)
    inc[:, 0:3], inc[:, 6:9] = (0, -1, 0), (0, 1, 0)
    sun = stock_sun(oracle)
    orc = oracle.Oracle()
    for field, m in offenders():
        for at in (0, 2):
            with pytest.raises(RuntimeError) as e:
                orc.upload(domain_scene(oracle, m, at))
            assert "sphere %d" % at in str(e.value) and "field " + field in str(e.value), str(e.value)
        if int(m["type"][0]) == EMISSIVE or field in ("type", "tex_type"):
            with pytest.raises(RuntimeError) as e:
                orc.upload(domain_scene(oracle, sky=m))
            assert "sky" in str(e.value) and "field " + field in str(e.value), str(e.value)
        for call in (lambda: oracle.scatter_n(m, in17_of(inc)), lambda: oracle.emit_shade_n(m, sun, STOCK_VIEW, hits8_of(inc))):
            with pytest.raises(RuntimeError) as e:
                call()
            assert "field " + field in str(e.value), str(e.value)
        mm = oracle.RtMaterial.from_buffer_copy(m.tobytes())
        f3 = lambda v: (C.c_float * 3)(*v)
        att, dr, nd, loc = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint32(), (C.c_float * 3)()
        assert oracle.lib().orc_unit_scatter(C.byref(mm), f3((0, -1, 0)), f3((0, 0, 0)), f3((0, 1, 0)), (C.c_float * 2)(0.5, 0.5), f3((0.5, 0.5, 0.5)), att, dr, C.byref(nd)) == -1
        oracle.lib().orc_unit_emit_shade(C.byref(mm), C.byref(sun), f3(STOCK_VIEW), f3((0, 0, 0)), f3((0, 1, 0)), (C.c_float * 2)(0.5, 0.5), loc)
        assert all(np.isnan(v) for v in loc)
        if field in ("tex_type", "rgb0", "rgb1", "tiling"):
            with pytest.raises(RuntimeError) as e:
                oracle.texture_eval(m, np.array([[0.25, 0.75]], F))
            assert "field " + field in str(e.value), str(e.value)
    for m in unread_nan_records():
        orc.upload(domain_scene(oracle, m, 1))
        orc.render(16, 8, 1, 2, 4, 1)
        assert np.isfinite(orc.download()[0]).all()
        assert np.isfinite(oracle.scatter_n(m, in17_of(inc))).all()
        oracle.emit_shade_n(m, sun, STOCK_VIEW, hits8_of(inc))
    # the largest tiling inside the domain, at the uv corner where the product is largest
    m = _record(OPAQUE, CHECKER, smoothness=16.0, tiling=2.0 ** 30)
    assert np.isfinite(oracle.texture_eval(m, np.array([[1.0, 1.0], [np.nextafter(F(1), F(2)), 0.0]], F))).all()
    orc.close()


def test_generated_records_cover_the_issue_values():
    recs = material_records()
    assert 50 <= len(recs) <= 70
    for kind in (OPAQUE, METAL, EMISSIVE):
        mine = [m for m in recs if int(m["type"][0]) == kind]
        assert {int(m["tex_type"][0]) for m in mine} == {CONST, CHECKER}
        assert {float(m["tiling"][0]) for m in mine if int(m["tex_type"][0]) == CHECKER} == {float(F(t)) for t in TILING}
    for kind in (OPAQUE, METAL, GLASS):
        assert {float(m["smoothness"][0]) for m in recs if int(m["type"][0]) == kind} == {float(F(s)) for s in SMOOTHNESS}
    assert {float(m["ior"][0]) for m in recs if int(m["type"][0]) == GLASS} == {float(F(i)) for i in IOR}
    assert {float(m["luminance"][0]) for m in recs if int(m["type"][0]) == EMISSIVE} == {float(F(l)) for l in LUMINANCE}
    bytes_ = np.concatenate([np.rint(m["rgb0"][0] * 255.0) for m in recs] + [np.rint(m["rgb1"][0] * 255.0) for m in recs])
    assert 0 in bytes_ and 255 in bytes_
    for m in recs:  # byte colours only
        for c in list(m["rgb0"][0]) + list(m["rgb1"][0]):
            assert F(np.rint(c * 255.0)) * K255 == c
    assert len({record_id(m) for m in recs}) == len(recs)
