"""Device hit processing (rt_shade.h scatter_only / shade_only / shade_value, the material loaders, eval_texture) against the oracle
over the material and incidence space of tests/test_hit_processing_cpu.py, bit for bit: at unit level through rt_unit_scatter
and rt_unit_math, and through the production kernels (rt_unit_closest_hit, rt_unit_trace, rt_render) on "material chart"
scenes that carry one sphere per record -- the 48-byte records, packed records from LDS and from global memory, and the
several-lights branch.  No tolerance anywhere: a NaN is compared as "a NaN in the same place", the attenuation and direction
of a hit that does not scatter are unspecified in the reference and masked, and both kinds of exemption are capped."""
import ctypes as C
import re

import numpy as np
import pytest

import test_hit_processing_cpu as G
from test_gpu_parity import _assert_image_equals_oracle, _custom_scene, assert_same, bits

pytestmark = pytest.mark.gpu

F = np.float32
RECORDS = G.material_records()
RECORD_IDS = [G.record_id(m) for m in RECORDS]


def assert_same_or_nan_alike(got, want, what):
    """bit for bit; where the oracle has a NaN the device must have one too (any payload), and nowhere else"""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaNs in other places, %d device vs %d oracle, first row %d" % (
        what, int(gn.sum()), int(wn.sum()), int(np.argmax((gn != wn).any(axis=1))))
    g, w = np.where(gn, F(0), got), np.where(wn, F(0), want)
    if not np.array_equal(bits(g), bits(w)):
        bad = (bits(g) != bits(w)).any(axis=1)
        k = int(np.argmax(bad))
        raise AssertionError("%s: %d of %d rows differ, first row %d: device %r oracle %r" % (what, int(bad.sum()), len(bad), k, got[k], want[k]))


def device_scatter(hip, record, sun, view_origin, inc):
    from cpuraytracer_amd import _capi
    out = np.zeros((inc.shape[0], 11), dtype=F)
    mm = _capi.RtMaterial.from_buffer_copy(record.tobytes())
    ss = _capi.RtLight.from_buffer_copy(bytes(sun))
    view = (C.c_float * 3)(*view_origin)
    _capi.check(hip._L.rt_unit_scatter(hip._h, C.byref(mm), C.byref(ss), view, inc.ctypes.data, inc.shape[0], out.ctypes.data))
    return out


# ------------------------------------------------------------------------- unit level
@pytest.mark.parametrize("r", range(len(RECORDS)), ids=RECORD_IDS)
def test_unit_scatter_and_shade_over_the_incidence_space(hip, oracle, r):
    """rt_unit_scatter against scatter_n + orc_unit_emit_shade_n for one record: its 4,096 incidences x 3 view origins x 5 suns,
    under sampler flags 0, 1, 2, 3."""
    m = RECORDS[r]
    kind = int(m["type"][0])
    inc = G.incidences(oracle, m)
    h8 = G.hits8_of(inc)
    sun_list = G.suns(oracle)
    shade = {(v, s): oracle.emit_shade_n(m, sun_list[s], G.VIEW_ORIGINS[v], h8) for v in range(len(G.VIEW_ORIGINS)) for s in range(len(sun_list))}
    n_nan = n_cases = 0
    try:
        for flags in (0, 1, 2, 3):
            hip.set_sampler(flags)
            oracle.lib().orc_set_sampler(flags)
            scat = G.oracle_scatter11(oracle, m, inc)
            masked = (scat[:, 0] == 0) if kind in (G.OPAQUE, G.METAL) else np.zeros(len(inc), bool)
            assert masked.mean() <= G.MAX_UNSCATTERED
            for (v, s), local in shade.items():
                want = np.concatenate([scat, local], 1)
                got = device_scatter(hip, m, sun_list[s], G.VIEW_ORIGINS[v], inc)
                assert np.array_equal(got[:, 0], want[:, 0]), "%s: scattered flags differ" % RECORD_IDS[r]
                got[masked, 1:7] = 0
                want[masked, 1:7] = 0
                assert_same_or_nan_alike(got, want, "%s, sampler %d, view origin %d, sun %d" % (RECORD_IDS[r], flags, v, s))
                n_nan += int(np.isnan(want).any(axis=1).sum())
                n_cases += len(want)
    finally:
        hip.set_sampler(0)
        oracle.lib().orc_set_sampler(0)
    print("%s: %d cases, %d with a NaN" % (RECORD_IDS[r], n_cases, n_nan))
    assert n_nan <= G.MAX_NAN * n_cases


def pow_inputs(y, rng):
    """x in [0, 1] for rt_powf(x, y), about 300,000: uniform, and (a uniform x to the power 2048 is 0 nearly always) x chosen so that
    x^y is spread over the normal range; every float within 64 ulp of 0 and of 1; and x chosen so that x^y runs through the
    binary32 subnormals into underflow (results from 2^-120 down to 2^-160)"""
    ulps = np.arange(65, dtype=np.uint32)
    near0 = ulps.view(F)                                                 # 0 and the 64 smallest subnormals
    near_min_normal = (np.uint32(0x00800000) + ulps - np.uint32(32)).view(F)
    near1 = (np.uint32(0x3f800000) - ulps).view(F)
    parts = [rng.uniform(0, 1, 180000), near0, near_min_normal, near1, [0.5, 0.25, 1e-30, 1e-45]]
    if y > 0:
        parts.append(np.exp2(rng.uniform(-126.0, 0.0, 100000) / y))
        parts.append(np.exp2(rng.uniform(-160.0, -120.0, 20000) / y))
        parts.append(np.exp2(np.array([-126.0, -127.0, -148.0, -149.0, -149.5, -150.0, -151.0]) / y))
    x = np.concatenate([np.asarray(p, np.float64) for p in parts])
    return np.clip(x, 0.0, 1.0).astype(F)


@pytest.mark.parametrize("y", sorted({float(m["smoothness"][0]) for m in RECORDS}))
def test_powf_at_the_smoothness_exponents(hip, oracle, y):
    """rt_unit_math op 2 at every smoothness of the material space (test_elementary_functions_device_vs_oracle stops at y = 40)"""
    rng = np.random.default_rng(int(y * 2) + 17)
    x = pow_inputs(y, rng)
    yy = np.full_like(x, F(y))
    want = oracle.math_array(2, x, yy)
    if y >= 1:
        sub = (want > 0) & (want < F(2.0 ** -126))
        assert sub.sum() >= 1000 and (want == 0).sum() >= 1000, "the inputs do not reach the subnormals and the underflow"
    assert_same_or_nan_alike(hip.unit_math(2, x, yy).reshape(-1, 1), want.reshape(-1, 1), "pow y=%g" % y)


# ------------------------------------------------------------------------- production kernels
CHART_W, CHART_H, CHART_RAYS = 1140, 20, 3000  # the (virtual) image of the seeded primary rays; the camera's aspect is its own
SPACING, RADIUS = 1.02, 0.5


def chart_scene(oracle, rows=1, filler=0, n_lights=1):
    """One row of small spheres on a floor, one per record, then a hollow glass shell (an inner sphere of negative radius inside an
    outer one); a far camera whose frame the row fills.  rows: so many rows in all, the further ones behind the first (they take no
    primary hit from it); a scene of eight rows is still a flat scan, and large enough for the launcher to move the material table
    out of LDS.  filler: so many more spheres far behind the camera's view (beyond 512 spheres: tables in global memory)."""
    n = len(RECORDS) + 1
    xs = (np.arange(n) - 0.5 * (n - 1)) * SPACING
    centers = np.stack([xs, np.zeros(n), np.zeros(n)], 1)
    radii = np.full(n, RADIUS)
    centers = np.concatenate([centers, centers[-1:], [[0.0, -1000.0 - RADIUS, 0.0]]])
    radii = np.concatenate([radii, [-0.8 * RADIUS], [1000.0]])
    for row in range(1, rows):
        centers = np.concatenate([centers, np.stack([xs, np.zeros(n), np.full(n, row * SPACING)], 1)])
        radii = np.concatenate([radii, np.full(n, RADIUS)])
    if filler:
        rng = np.random.default_rng(filler)
        fc = np.stack([rng.uniform(-300, 300, filler), rng.uniform(0, 50, filler), rng.uniform(4000, 4600, filler)], 1)
        centers = np.concatenate([centers, fc])
        radii = np.concatenate([radii, rng.uniform(0.3, 0.6, filler)])
    types = np.zeros(len(radii), dtype=np.uint32)
    width = n * SPACING
    dist = 300.0
    vfov = float(np.degrees(2.0 * np.arctan(0.5 * 1.04 * 2.0 * RADIUS / dist)))
    sc = _custom_scene(oracle, centers.astype(F), radii.astype(F), types, (0.0, 6.0, -dist), (0.0, 0.0, 0.0), vfov, width / (1.04 * 2.0 * RADIUS))
    for k, m in enumerate(RECORDS):
        sc.materials[k] = m[0]
    shell = G._record(G.GLASS, smoothness=35.5, ior=1.5)[0]
    sc.materials[n - 1] = shell
    sc.materials[n] = shell
    for k in range(n + 2, len(radii)):
        sc.materials[k] = RECORDS[(k * 7) % len(RECORDS)][0]
    if n_lights > 1:
        sc.lights = [sc.sun, oracle.make_light((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0), oracle.make_light((0.3, -1.0, 0.2), (1.0, 0.2, 0.2), 30000.0)][:n_lights]
    return sc


def chart_rays(orc):
    rng = np.random.default_rng(4242)
    ijs = np.stack([rng.integers(0, CHART_W, CHART_RAYS), rng.integers(0, CHART_H, CHART_RAYS), rng.integers(1, 600, CHART_RAYS)], 1).astype(np.uint32)
    return ijs, orc.primary_rays(CHART_W, CHART_H, ijs)


LAUNCH_LINE = re.compile(r"rt_trace launch: tree=(\d+) flat=(\d+) ldsTables=(\d+) blocks=\d+ threads=(\d+) lds=(\d+) B \(cand (\d+), tables (\d+), leaf (\d+), "
                         r"ops (\d+), sg (\d+), tree (\d+), cache (\w+), stash (\d+)\)")
STASH_RECORD_BYTES = 76  # rt_kernels.h kStashDwords * 4


def launch_paths(stderr_text, rt_mats16):
    """(scan, materials) of every trace launch in the RT_VERBOSE lines of a run, read off the launcher's own account of its LDS
    image.  scan: "flat", "tree" or "grid" (tables in global memory for the last two).  materials, for the flat scan with its hit
    stash: the image is cand + tables + leaf + ops + sg + tree (rounded to 16 bytes) plus the stash (per wave, its records rounded
    to 16 bytes), where `tables` holds 72 bytes per scan entry, 48 of them the material record.  What the launch asks for beyond
    that sum is 0 -- "48-byte records in LDS" --, minus 48 bytes per entry -- the table is read through L2: "48-byte records
    from global memory", or with RT_MATS16 >= 1 "packed records from global memory" (mats16_mode 1) --, or minus 32 per entry --
    the table left and its 16-byte form came in: "packed records in LDS" (mats16_mode 2).  Anything else fails here.  The tree and
    grid scans read their materials from global memory: the packed records (mode 1) exactly when RT_MATS16 >= 1."""
    out = []
    for mt in LAUNCH_LINE.finditer(stderr_text):
        tree, flat, _, threads, total, cand, tables, leaf, ops, sg, treeb = (int(mt.group(k)) for k in range(1, 12))
        cache, cap = mt.group(12), int(mt.group(13))
        from_global = "packed records from global memory" if rt_mats16 >= 1 else "48-byte records from global memory"
        if tree or flat in (2, 3):  # (flat = 1 flat + 2 grid + 4 grid with its tables in LDS)
            out.append(("tree" if tree else "grid", from_global))
            continue
        assert flat == 1 and cap > 0 and cache == "no", "not the flat scan with the hit stash: " + mt.group(0)
        assert tables % 72 == 0
        entries = tables // 72
        image = (cand + tables + leaf + ops + sg + treeb + 15) // 16 * 16
        stash = (threads // 64) * ((cap * STASH_RECORD_BYTES + 15) // 16 * 16)
        extra = total - image - stash
        kinds = {0: "48-byte records in LDS", -48 * entries: from_global, -32 * entries: "packed records in LDS"}
        assert extra in kinds, "the launch's LDS image is not accounted for (%d bytes beyond the sum, %d entries): %s" % (extra, entries, mt.group(0))
        out.append(("flat", kinds[extra]))
    return out


# RT_MATS16 is 0 by default (the 48-byte records); 1 reads the packed records from global memory wherever the 48-byte table would be
# read from there, 2 also stages them into LDS in the flat scan once the scene is large enough for the material table to leave LDS
# (rt_capi.hip).  Between them the variants load a material every way the production kernels can; `path` is what every trace
# launch of the variant must report (launch_paths).
CHARTS = {
    "as-is": dict(env={}, rows=1, filler=0, n_lights=1, path=("flat", "48-byte records in LDS")),
    "records-through-l2": dict(env={}, rows=8, filler=0, n_lights=1, path=("flat", "48-byte records from global memory")),
    "packed-lds": dict(env={"RT_MATS16": "2"}, rows=8, filler=0, n_lights=1, path=("flat", "packed records in LDS")),
    "global-tables": dict(env={}, rows=1, filler=600, n_lights=1, path=("tree or grid", "48-byte records from global memory")),
    "global-tables-packed": dict(env={"RT_MATS16": "1"}, rows=1, filler=600, n_lights=1, path=("tree or grid", "packed records from global memory")),
    "three-lights": dict(env={}, rows=1, filler=0, n_lights=3, path=("flat", "48-byte records in LDS")),
    "three-lights-packed": dict(env={"RT_MATS16": "2"}, rows=8, filler=0, n_lights=3, path=("flat", "packed records in LDS")),
}


@pytest.mark.parametrize("flags", [0, 3], ids=["sampler0", "sampler3"])
@pytest.mark.parametrize("chart", sorted(CHARTS))
def test_material_chart_through_the_production_kernels(hip, oracle, monkeypatch, capfd, chart, flags):
    """The material space through rt_unit_closest_hit, rt_unit_trace (depth 0, 1, 30) and rt_render on a chart scene: as is (flat
    scan, the 48-byte records in LDS); eight rows deep, where the launcher reads the 48-byte records through L2 and, RT_MATS16=2,
    stages the packed records into LDS; padded with far-away spheres beyond 512 (tables in global memory; 48-byte and, RT_MATS16=1,
    packed records from there); under three lights (the several-lights branch, with either record form).  Every trace launch must
    report the path its variant names."""
    from cpuraytracer_amd import HipRenderer
    cfg = CHARTS[chart]
    sc = chart_scene(oracle, cfg["rows"], cfg["filler"], cfg["n_lights"])
    orc = oracle.Oracle()
    orc.upload(sc)
    ijs, rays = chart_rays(orc)
    hits = orc.closest_hit(rays, oracle.ACCEL_PADDED_LIST)
    idx = hits[:, 1].copy().view(np.int32)
    per_record = np.bincount(idx[idx >= 0], minlength=sc.n)[:len(RECORDS) + 1]
    assert per_record.min() >= 20, "a record's sphere receives %d primary hits" % per_record.min()
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RT_VERBOSE", "1")
    dev = HipRenderer(0) if cfg["env"] else hip
    try:
        dev.set_sampler(flags)
        oracle.lib().orc_set_sampler(flags)
        dev.upload(sc)
        assert_same(dev.unit_primary_rays(CHART_W, CHART_H, ijs), rays, "primary rays")
        assert_same(dev.unit_closest_hit(rays), hits, "closest hits")
        capfd.readouterr()
        for depth in (0, 1, 30):
            rg, tg = dev.unit_trace(CHART_W, CHART_H, ijs, depth, 91)
            ro, to = orc.trace(CHART_W, CHART_H, ijs, depth, 91, accel=oracle.ACCEL_PADDED_LIST)
            assert_same_or_nan_alike(rg, ro, "per-sample radiance, depth %d" % depth)
            assert np.array_equal(tg, to), "traversal counts, depth %d" % depth
            assert np.isnan(ro).any(axis=1).mean() <= G.MAX_NAN
        _assert_image_equals_oracle(dev, oracle, sc, 160, 100, 2, 20)
        paths = launch_paths(capfd.readouterr().err, int(cfg["env"].get("RT_MATS16", "0")))
        assert len(paths) >= 4, "the trace launches did not report themselves"
        want_scan, want_mats = cfg["path"]
        for scan, mats in paths:
            assert (scan in ("tree", "grid") if want_scan == "tree or grid" else scan == want_scan) and mats == want_mats, (chart, paths)
    finally:
        dev.set_sampler(0)
        oracle.lib().orc_set_sampler(0)
        if dev is not hip:
            dev.close()


# ------------------------------------------------------------------------- the material domain
def test_upload_and_unit_scatter_refuse_records_outside_the_material_domain(hip, oracle):
    """rt_scene_upload refuses every offender of the CPU file's list exactly as orc_scene_upload does -- RT_ERR_INVALID_ARG, the
    sphere (or the sky) and the field named -- before any side effect: the scene uploaded before still renders the same bits.
    rt_unit_scatter refuses the same records; NaN in fields a type does not read is accepted by both."""
    from cpuraytracer_amd import RtError
    good = G.domain_scene(oracle)
    hip.upload(good)
    hip.render(64, 32, 1, 3, 8, 5)
    before = hip.download(ldr=False)[0]
    orc = oracle.Oracle()
    inc = np.zeros((4, 12), F)
    inc[:, 0:3], inc[:, 6:9] = (0, -1, 0), (0, 1, 0)
    sun = G.stock_sun(oracle)
    for field, m in G.offenders():
        scenes = [("sphere 1", G.domain_scene(oracle, m, 1))]
        if int(m["type"][0]) == G.EMISSIVE or field in ("type", "tex_type"):
            scenes.append(("sky", G.domain_scene(oracle, sky=m)))
        for what, sc in scenes:
            with pytest.raises(RtError) as e:
                hip.upload(sc)
            assert e.value.code == 2 and what in str(e.value) and field in str(e.value), str(e.value)
            with pytest.raises(RuntimeError) as eo:
                orc.upload(sc)
            assert what in str(eo.value) and field in str(eo.value)
        with pytest.raises(RtError) as e:
            device_scatter(hip, m, sun, G.STOCK_VIEW, inc)
        assert e.value.code == 2 and field in str(e.value), str(e.value)
        hip.render(64, 32, 1, 3, 8, 5)
        assert_same(hip.download(ldr=False)[0], before, "the scene uploaded before the refused one (%s)" % field)
    # a refused upload in the middle of an accumulation leaves the accumulation alone
    hip.render(64, 32, 1, 2, 8, 5)
    with pytest.raises(RtError):
        hip.upload(G.domain_scene(oracle, G.offenders()[0][1], 0))
    hip.render(64, 32, 2, 3, 8, 5)
    assert_same(hip.download(ldr=False)[0], before, "an accumulation continued across a refused upload")
    for m in G.unread_nan_records():
        sc = G.domain_scene(oracle, m, 1)
        _assert_image_equals_oracle(hip, oracle, sc, 48, 24, 2, 8)
        want = np.concatenate([G.oracle_scatter11(oracle, m, inc), oracle.emit_shade_n(m, sun, G.STOCK_VIEW, G.hits8_of(inc))], 1)
        assert_same_or_nan_alike(device_scatter(hip, m, sun, G.STOCK_VIEW, inc), want, "NaN in unread fields")


def test_device_and_oracle_refuse_the_same_random_records(hip, oracle):
    """The domain rule is written twice (rtprep::MaterialFault for the device library, a restatement in the oracle): 20,000 random
    records -- types and texture kinds in and out of range, every float field drawn from finite values, NaN, the infinities and
    tilings either side of 2^30 -- must be accepted or refused alike, with the same field named.  rt_unit_scatter and
    orc_unit_scatter_n with n = 0 apply the rule and do nothing else."""
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(77)
    n = 20000
    pool = np.array([0.0, 0.5, 1.0, 16.0, -50.0, 2500.0, 2.0 ** 30, -(2.0 ** 30), np.nextafter(F(2.0 ** 30), F(np.inf)), -3.0e9, 3.4e38,
                     np.nan, np.inf, -np.inf], F)
    finite = np.isfinite(pool)
    def draw(shape):  # mostly finite, so that many records get past the first clauses
        return np.where(rng.random(shape) < 0.85, rng.choice(pool[finite], shape), rng.choice(pool, shape)).astype(F)
    recs = np.zeros(n, dtype=G.MATERIAL_DTYPE)
    recs["type"] = rng.choice(np.array([0, 1, 2, 3, 0, 1, 2, 3, 4, 0xffffffff], np.uint32), n)
    recs["tex_type"] = rng.choice(np.array([0, 1, 0, 1, 0, 1, 2, 7], np.uint32), n)
    for f in ("smoothness", "ior", "tiling", "luminance"):
        recs[f] = draw(n)
    recs["rgb0"], recs["rgb1"] = draw((n, 3)), draw((n, 3))
    sun = _capi.RtLight.from_buffer_copy(bytes(G.stock_sun(oracle)))
    view = (C.c_float * 3)(*G.STOCK_VIEW)
    dummy = np.zeros(17, F)
    refused = {}
    for k in range(n):
        raw = recs[k:k + 1].tobytes()
        md, mo = _capi.RtMaterial.from_buffer_copy(raw), oracle.RtMaterial.from_buffer_copy(raw)
        rc_dev = hip._L.rt_unit_scatter(hip._h, C.byref(md), C.byref(sun), view, dummy.ctypes.data, 0, dummy.ctypes.data)
        rc_orc = oracle.lib().orc_unit_scatter_n(C.byref(mo), dummy.ctypes.data, 0, 0, dummy.ctypes.data)
        assert rc_dev in (0, 2) and (rc_dev == 2) == (rc_orc != 0), (recs[k], rc_dev, rc_orc)
        if rc_orc:
            field = oracle.lib().orc_last_error().decode().rsplit("field ", 1)[1]
            msg = hip._L.rt_last_error().decode()
            assert ": %s " % field in msg, (field, msg)
            refused[field] = refused.get(field, 0) + 1
    print("refused by field:", refused, "accepted:", n - sum(refused.values()))
    assert set(refused) == {"type", "tex_type", "smoothness", "ior", "luminance", "rgb0", "rgb1", "tiling"} and n - sum(refused.values()) >= 2000
