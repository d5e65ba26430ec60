// temporal_shards_selftest.cpp -- the sharded temporal twin (rt_unit_temporal_shards_host, rt_temporal_host.cpp over ../rt_rowset_map.h
// and ../rt_temporal.h) in a program of its own: random shardings, bands of the image, histories and pairs of cameras.  No HIP, no
// librt_hip.so; also built under ASan + UBSan (Makefile temporal_shards_selftest_san), where every index the mapping forms is checked:
// the parts are exactly nshards * rows_max * W pixels long.  Each case cuts a random strip into the parts of a random sharding --
// padding rows NaN, padding ids 0xffffffff -- and against the contiguous twin (rt_unit_temporal_host_fetch) over the strip itself:
//   - rgb, var, state, guides, len and target are the same bytes, for both fetches, with a history and without;
//   - a larger rows_max (more padding) changes nothing;
//   - an empty history gives rt_unit_denoise_shards_host's bytes;
//   - the refusals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../../include/rt_api.h"
#include "../rt_rowset_map.h"
#include "../rt_temporal.h"
#include "rt_denoise_host.h"
#include "rt_error.h"

namespace rtprep {
static thread_local std::string g_err;
int Fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
const char* LastError() { return g_err.c_str(); }
}  // namespace rtprep

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);            \
            std::fprintf(stderr, "\n");                   \
            if (++g_fail > 20) std::exit(1);              \
        }                                                 \
    } while (0)

struct Frame {
    uint32_t n, m;
    std::vector<float> hdr, sq, feat;
    std::vector<uint32_t> ids;
};

// Guides and ids that vary slowly over the strip, so that under a small camera move most pixels pass the validation.
static Frame RandomFrame(std::mt19937& rng, uint32_t W, uint32_t rows) {
    const size_t npix = (size_t)W * rows;
    Frame s;
    s.n = 2 + rng() % 6;
    s.m = 1 + rng() % 4;
    s.hdr.resize(npix * 3);
    s.sq.resize(npix * 3);
    s.feat.resize(npix * 8);
    s.ids.resize(npix);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    const uint32_t cut = 1 + rng() % W;
    for (size_t p = 0; p < npix; ++p) {
        for (int c = 0; c < 3; ++c) {
            float S = 0.f, Q = 0.f;
            for (uint32_t k = 0; k < s.n; ++k) {
                const float v = 4.f * u(rng) * u(rng);
                S += v;
                Q += v * v;
            }
            s.hdr[3 * p + c] = S;
            s.sq[3 * p + c] = Q;
        }
        const bool sky = (p % W) >= cut;
        const float fm = (float)s.m;
        float* f = &s.feat[8 * p];
        for (int c = 0; c < 3; ++c) f[c] = u(rng) * fm;
        for (int c = 3; c < 6; ++c) f[c] = sky ? 0.f : (0.2f * u(rng) - 0.1f) * fm;
        f[7] = sky ? 0.f : fm;
        f[6] = sky ? 0.f : (12.f + 0.05f * u(rng)) * f[7];
        s.ids[p] = sky ? 0xffffffffu : 1u + (uint32_t)(rng() % 16 == 0);
    }
    return s;
}

// The parts of a strip: row ly of it goes where the mapping says, everything else is padding.
static Frame CutIntoParts(const Frame& s, uint32_t W, uint32_t rows, uint32_t block_rows, uint32_t nshards, uint32_t rows_max) {
    const size_t px = (size_t)nshards * rows_max * W;
    Frame parts;
    parts.n = s.n;
    parts.m = s.m;
    parts.hdr.assign(px * 3, NAN);
    parts.sq.assign(px * 3, NAN);
    parts.feat.assign(px * 8, NAN);
    parts.ids.assign(px, 0xffffffffu);
    for (uint32_t ly = 0; ly < rows; ++ly) {
        uint32_t shard, lr;
        rtd::rowset_locate(block_rows, nshards, ly, shard, lr);
        const size_t src = (size_t)ly * W, dst = ((size_t)shard * rows_max + lr) * W;
        std::memcpy(&parts.hdr[3 * dst], &s.hdr[3 * src], (size_t)W * 12);
        std::memcpy(&parts.sq[3 * dst], &s.sq[3 * src], (size_t)W * 12);
        std::memcpy(&parts.feat[8 * dst], &s.feat[8 * src], (size_t)W * 32);
        std::memcpy(&parts.ids[dst], &s.ids[src], (size_t)W * 4);
    }
    return parts;
}

// A pinhole record looking from `from` at the origin, as Camera::Camera lays it out (x = halfWidth u, y = halfHeight v).
static rt_camera LookAtOrigin(const float from[3], float halfW, float halfH) {
    float w[3], len = 0.f;
    for (int k = 0; k < 3; ++k) len += from[k] * from[k];
    len = std::sqrt(len);
    for (int k = 0; k < 3; ++k) w[k] = -from[k] / len;
    float u[3] = {w[2], 0.f, -w[0]};  // up x w, up = (0, 1, 0)
    float ul = std::sqrt(u[0] * u[0] + u[2] * u[2]);
    if (!(ul > 1e-6f)) u[0] = 1.f, u[2] = 0.f, ul = 1.f;
    for (int k = 0; k < 3; ++k) u[k] /= ul;
    const float v[3] = {w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]};
    rt_camera c;
    std::memset(&c, 0, sizeof c);
    for (int k = 0; k < 3; ++k) {
        c.origin[k] = from[k];
        c.x[k] = halfW * u[k];
        c.y[k] = halfH * v[k];
        c.origin_image_plane[k] = from[k] + w[k];
    }
    return c;
}

struct Out {
    std::vector<float> rgb, var, st, og;
    std::vector<uint32_t> len, tgt;
    explicit Out(size_t npix) : rgb(npix * 3, NAN), var(npix, NAN), st(npix * 4, NAN), og(npix * 8, NAN), len(npix, 12345u), tgt(npix, 12345u) {}
    bool SameBytes(const Out& o) const {
        return std::memcmp(rgb.data(), o.rgb.data(), rgb.size() * 4) == 0 && std::memcmp(var.data(), o.var.data(), var.size() * 4) == 0 &&
               std::memcmp(st.data(), o.st.data(), st.size() * 4) == 0 && std::memcmp(og.data(), o.og.data(), og.size() * 4) == 0 && len == o.len && tgt == o.tgt;
    }
};

static rt_shard_frame ShapeOf(uint32_t W, uint32_t H, uint32_t first, uint32_t rows, uint32_t block_rows, uint32_t nshards, uint32_t rows_max, uint32_t n,
                              uint32_t m, const rt_camera& C) {
    rt_shard_frame f;
    std::memset(&f, 0, sizeof f);
    f.parts.W = W;
    f.parts.rows_max = rows_max;
    f.parts.rs = rt_rowset{first, rows, block_rows, 0, nshards};
    f.parts.n = n;
    f.parts.m = m;
    f.H = H;
    f.camera = C;
    return f;
}

int main(int argc, char** argv) {
    const uint32_t cases = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 300u;
    std::mt19937 rng(20261020u);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    size_t pixels = 0, accepted = 0, moved = 0, padded = 0;
    for (uint32_t t = 0; t < cases; ++t) {
        const uint32_t W = 1 + rng() % (t % 10 == 0 ? 90 : 24), H = 1 + rng() % (t % 10 == 1 ? 70 : 20);
        const uint32_t first = rng() % 3 == 0 ? rng() % H : 0, rows = rng() % 3 == 0 ? 1 + rng() % (H - first) : H - first;
        const uint32_t nshards = 1 + rng() % (t % 7 == 0 ? 12 : 4), block_rows = 1 + rng() % (t % 5 == 0 ? rows + 2 : 4);
        const uint32_t most = rtd::rowset_max_shard_rows(rows, block_rows, nshards);
        const size_t npix = (size_t)W * rows;
        const uint32_t fetch = t % 2 ? RT_TEMPORAL_FETCH_BILINEAR : RT_TEMPORAL_FETCH_NEAREST;
        const Frame cur = RandomFrame(rng, W, rows);
        rt_temporal_params T;
        rt_temporal_default_params_fetch(fetch, &T);
        T.max_history = 1 + rng() % 64;
        T.use_id = rng() % 2;
        T.depth_tol = 0.9f;
        std::vector<float> hs(npix * 4), hg(npix * 8);
        std::vector<uint32_t> hl(npix);
        for (size_t p = 0; p < npix; ++p) {
            for (int k = 0; k < 4; ++k) hs[4 * p + k] = 2.f * u(rng);
            for (int k = 0; k < 8; ++k) hg[8 * p + k] = cur.feat[8 * p + k] / (float)cur.m;
            hl[p] = rng() % 8 ? 1 + rng() % 69 : rng() % 70;  // 0: a pixel that holds nothing
        }
        const float from[3] = {20.f * u(rng) - 10.f, 6.f * u(rng) - 1.f, 20.f * u(rng) - 10.f};
        float from2[3];
        const uint32_t move = t % 3;  // 0 the same camera, 1 a small move, 2 anywhere
        for (int k = 0; k < 3; ++k) from2[k] = move == 0 ? from[k] : (move == 1 ? from[k] + 0.2f * u(rng) - 0.1f : 20.f * u(rng) - 10.f);
        const float hw = 0.2f + u(rng), hh = hw * (float)H / (float)W;
        const rt_camera C = LookAtOrigin(from, hw, hh), Cp = LookAtOrigin(from2, hw, hh);
        rt_denoise_params P;
        rt_denoise_default_params(&P);
        P.levels = 1 + rng() % 3;

        Out want(npix), wantEmpty(npix);
        int rc = rt_unit_temporal_host_fetch(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, &Cp, hs.data(),
                                             hg.data(), cur.ids.data(), hl.data(), &P, &T, fetch, want.rgb.data(), want.var.data(), want.st.data(), want.og.data(),
                                             want.len.data(), want.tgt.data());
        CHECK(rc == RT_OK, "case %u, contiguous: rc %d (%s)", t, rc, rtprep::LastError());
        rc = rt_unit_temporal_host_fetch(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, &P, &T, fetch, wantEmpty.rgb.data(), wantEmpty.var.data(), wantEmpty.st.data(),
                                         wantEmpty.og.data(), wantEmpty.len.data(), wantEmpty.tgt.data());
        CHECK(rc == RT_OK, "case %u, contiguous, empty history: rc %d (%s)", t, rc, rtprep::LastError());

        for (const uint32_t extra : {0u, 1u + (uint32_t)(rng() % 3)}) {
            const uint32_t rows_max = most + extra;
            const Frame parts = CutIntoParts(cur, W, rows, block_rows, nshards, rows_max);
            const rt_shard_frame shape = ShapeOf(W, H, first, rows, block_rows, nshards, rows_max, cur.n, cur.m, C);
            Out got(npix), gotEmpty(npix);
            rc = rt_unit_temporal_shards_host(parts.hdr.data(), parts.sq.data(), parts.feat.data(), parts.ids.data(), &shape, &Cp, hs.data(), hg.data(),
                                              cur.ids.data(), hl.data(), &P, &T, fetch, got.rgb.data(), got.var.data(), got.st.data(), got.og.data(),
                                              got.len.data(), got.tgt.data());
            CHECK(rc == RT_OK, "case %u, parts: rc %d (%s)", t, rc, rtprep::LastError());
            CHECK(got.SameBytes(want), "case %u (%u x %u rows %u..+%u of %u, %u shards of %u-row blocks, rows_max %u, fetch %u): parts != contiguous", t, W, rows,
                  first, rows, H, nshards, block_rows, rows_max, fetch);
            rc = rt_unit_temporal_shards_host(parts.hdr.data(), parts.sq.data(), parts.feat.data(), parts.ids.data(), &shape, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, &P, &T, fetch, gotEmpty.rgb.data(), gotEmpty.var.data(), gotEmpty.st.data(), gotEmpty.og.data(),
                                              gotEmpty.len.data(), gotEmpty.tgt.data());
            CHECK(rc == RT_OK, "case %u, parts, empty history: rc %d (%s)", t, rc, rtprep::LastError());
            CHECK(gotEmpty.SameBytes(wantEmpty), "case %u: parts != contiguous on an empty history", t);
            std::vector<float> rgb(npix * 3, NAN), var(npix, NAN);
            rc = rt_unit_denoise_shards_host(parts.hdr.data(), parts.sq.data(), parts.feat.data(), &shape.parts, &P, rgb.data(), var.data());
            CHECK(rc == RT_OK, "case %u, filter over the parts: rc %d (%s)", t, rc, rtprep::LastError());
            CHECK(std::memcmp(rgb.data(), gotEmpty.rgb.data(), npix * 12) == 0 && std::memcmp(var.data(), gotEmpty.var.data(), npix * 4) == 0,
                  "case %u: empty history != rt_unit_denoise_shards_host", t);
            padded += (size_t)nshards * rows_max * W - npix;
        }
        for (size_t p = 0; p < npix; ++p) {
            CHECK(want.tgt[p] == 0xffffffffu || want.tgt[p] < npix, "case %u pixel %zu: target %u of %zu", t, p, want.tgt[p], npix);
            accepted += want.tgt[p] != 0xffffffffu;
            moved += want.tgt[p] != 0xffffffffu && want.tgt[p] != p;
            CHECK(wantEmpty.len[p] == 1 && wantEmpty.tgt[p] == 0xffffffffu, "case %u pixel %zu: empty history blended", t, p);
        }
        pixels += npix;
    }
    CHECK(accepted > pixels / 20 && moved > pixels / 100, "%zu of %zu pixels accepted, %zu of them elsewhere: the cases do not exercise the gather", accepted, pixels,
          moved);
    CHECK(padded > pixels / 10, "only %zu padding pixels for %zu: the cases do not exercise the padding", padded, pixels);

    // refusals
    {
        const uint32_t W = 4, H = 7, first = 1, rows = 5, nshards = 2, rows_max = 3;
        const size_t npix = (size_t)W * rows;
        const Frame s = RandomFrame(rng, W, rows);
        const Frame f = CutIntoParts(s, W, rows, 1, nshards, rows_max);
        const float from[3] = {3.f, 1.f, 4.f};
        const rt_camera C = LookAtOrigin(from, 0.5f, 0.4f);
        std::vector<float> hs(npix * 4, 0.f), hg(npix * 8, 0.f), rgb(npix * 3), var(npix);
        std::vector<uint32_t> hl(npix, 1u), hid(npix, 1u);
        const rt_shard_frame good = ShapeOf(W, H, first, rows, 1, nshards, rows_max, 2, 1, C);
        auto call = [&](const rt_shard_frame& sh, const rt_camera* cp, const rt_denoise_params* P, const rt_temporal_params* T, uint32_t fetch) {
            return rt_unit_temporal_shards_host(f.hdr.data(), f.sq.data(), f.feat.data(), f.ids.data(), &sh, cp, hs.data(), hg.data(), hid.data(), hl.data(), P, T,
                                                fetch, rgb.data(), var.data(), nullptr, nullptr, nullptr, nullptr);
        };
        CHECK(call(good, &C, nullptr, nullptr, 4) == RT_OK, "the plain call: %s", rtprep::LastError());
        CHECK(call(good, &C, nullptr, nullptr, 1) == RT_OK, "the plain call, fetch 1: %s", rtprep::LastError());
        CHECK(rt_unit_temporal_shards_host(f.hdr.data(), f.sq.data(), f.feat.data(), nullptr, &good, &C, hs.data(), hg.data(), hid.data(), hl.data(), nullptr,
                                           nullptr, 1, rgb.data(), var.data(), nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID_ARG,
              "null ids");
        CHECK(rt_unit_temporal_shards_host(f.hdr.data(), f.sq.data(), f.feat.data(), f.ids.data(), nullptr, &C, hs.data(), hg.data(), hid.data(), hl.data(), nullptr,
                                           nullptr, 1, rgb.data(), var.data(), nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID_ARG,
              "null shape");
        CHECK(call(good, nullptr, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "a history without its camera");
        for (uint32_t bad : {0u, 2u, 3u, 5u, 0xffffffffu}) CHECK(call(good, &C, nullptr, nullptr, bad) == RT_ERR_INVALID_ARG, "fetch %u", bad);
        rt_shard_frame sh = good;
        sh.parts.n = 1;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_SEQUENCE, "n < 2");
        sh = good, sh.parts.m = 0;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_SEQUENCE, "m == 0");
        sh = good, sh.parts.W = 0;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "W == 0");
        sh = good, sh.parts.rs.num_rows = 0;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "no rows");
        sh = good, sh.parts.rs.nshards = 0;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "no shards");
        sh = good, sh.parts.rs.block_rows = 0;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "block_rows == 0");
        sh = good, sh.parts.rows_max = rows_max - 1;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "rows_max below the largest shard");
        sh = good, sh.H = first + rows - 1;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "rows beyond the image");
        sh = good, sh.H = (1u << 24) + 1u;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "H above 2^24");
        sh = good, sh.H = 1u << 24;
        CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_OK, "H of 2^24: %s", rtprep::LastError());
        for (int field = 0; field < 6; ++field)
            for (const float bad : {NAN, INFINITY, -INFINITY}) {
                sh = good;
                float* at[6] = {&sh.camera.origin[0], &sh.camera.x[1], &sh.camera.y[2], &sh.camera.origin_image_plane[1], &sh.camera.aperture, &sh.camera.focal_length};
                *at[field] = bad;
                CHECK(call(sh, &C, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "camera field %d = %g", field, bad);
            }
        rt_denoise_params P;
        rt_denoise_default_params(&P);
        P.levels = 6;
        CHECK(call(good, &C, &P, nullptr, 4) == RT_ERR_INVALID_ARG, "levels 6");
        rt_temporal_params def4, T;
        rt_temporal_default_params_fetch(RT_TEMPORAL_FETCH_BILINEAR, &def4);
        T = def4, T.max_history = 0;
        CHECK(call(good, &C, nullptr, &T, 4) == RT_ERR_INVALID_ARG, "max_history 0");
        T = def4, T.max_history = 65;
        CHECK(call(good, &C, nullptr, &T, 4) == RT_ERR_INVALID_ARG, "max_history 65");
        T = def4, T.depth_tol = -1.f;
        CHECK(call(good, &C, nullptr, &T, 4) == RT_ERR_INVALID_ARG, "negative tolerance");
        T = def4, T.normal_tol = NAN;
        CHECK(call(good, &C, nullptr, &T, 4) == RT_ERR_INVALID_ARG, "NaN tolerance");
        T = def4, T.coverage_tol = INFINITY;
        CHECK(call(good, &C, nullptr, &T, 4) == RT_ERR_INVALID_ARG, "infinite tolerance");
    }
    if (g_fail) {
        std::fprintf(stderr, "temporal_shards_selftest: %d failures\n", g_fail);
        return 1;
    }
    std::printf("temporal_shards_selftest ok: %u cases, %zu pixels, %zu accepted (%zu of them elsewhere), %zu padding pixels\n", cases, pixels, accepted, moved,
                padded);
    return 0;
}
