// denoise_shards_spatial_selftest.cpp -- the spatial variance source over the gathered parts of a row-sharded picture, both twins
// (rt_unit_denoise_shards_variance_host, rt_denoise_host.cpp; rt_unit_temporal_shards_variance_host, rt_temporal_host.cpp) in a program of
// its own.  No HIP, no librt_hip.so; also built under ASan + UBSan (Makefile denoise_shards_spatial_selftest_san), where every index the
// mapping forms is checked: the parts are exactly nshards * rows_max * W pixels long, and there is no sq buffer at all.  Each case cuts a
// seeded one-sample strip into the parts of a random sharding -- padding rows 0xff bytes, which are NaNs -- and against the contiguous
// twins (rt_unit_denoise_variance_host, rt_unit_temporal_variance_host) over the strip itself:
//   - rgb, var, the prepared state, and with the temporal step state, guides, len and target are the same bytes and finite, for radius
//     1..3 and both fetches, with a history and without;
//   - a larger rows_max (more padding) changes nothing;
//   - the moments source through the new twins gives the existing sharded twins' bytes;
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
    std::vector<float> hdr, sq, feat;  // sq: only where n >= 2 (the moments-source cases)
    std::vector<uint32_t> ids;
};

// Guides and ids that vary slowly over the strip, so that under a small camera move most pixels pass the validation.
static Frame RandomFrame(std::mt19937& rng, uint32_t W, uint32_t rows, uint32_t n) {
    const size_t npix = (size_t)W * rows;
    Frame s;
    s.n = n;
    s.m = 1 + rng() % 4;
    s.hdr.resize(npix * 3);
    if (n >= 2) s.sq.resize(npix * 3);
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
            if (n >= 2) s.sq[3 * p + c] = Q;
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

// The parts of a strip: row ly of it goes where the mapping says, everything else is padding of 0xff bytes.
static Frame CutIntoParts(const Frame& s, uint32_t W, uint32_t rows, uint32_t block_rows, uint32_t nshards, uint32_t rows_max) {
    const size_t px = (size_t)nshards * rows_max * W;
    Frame parts;
    parts.n = s.n;
    parts.m = s.m;
    parts.hdr.resize(px * 3);
    std::memset(parts.hdr.data(), 0xff, px * 12);
    if (!s.sq.empty()) {
        parts.sq.resize(px * 3);
        std::memset(parts.sq.data(), 0xff, px * 12);
    }
    parts.feat.resize(px * 8);
    std::memset(parts.feat.data(), 0xff, px * 32);
    parts.ids.assign(px, 0xffffffffu);
    for (uint32_t ly = 0; ly < rows; ++ly) {
        uint32_t shard, lr;
        rtd::rowset_locate(block_rows, nshards, ly, shard, lr);
        const size_t src = (size_t)ly * W, dst = ((size_t)shard * rows_max + lr) * W;
        std::memcpy(&parts.hdr[3 * dst], &s.hdr[3 * src], (size_t)W * 12);
        if (!s.sq.empty()) std::memcpy(&parts.sq[3 * dst], &s.sq[3 * src], (size_t)W * 12);
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

static bool AllFinite(const std::vector<float>& v) {
    for (const float x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

struct Out {
    std::vector<float> rgb, var, st, og;
    std::vector<uint32_t> len, tgt;
    explicit Out(size_t npix) : rgb(npix * 3, NAN), var(npix, NAN), st(npix * 4, NAN), og(npix * 8, NAN), len(npix, 12345u), tgt(npix, 12345u) {}
    bool SameBytes(const Out& o) const {
        return std::memcmp(rgb.data(), o.rgb.data(), rgb.size() * 4) == 0 && std::memcmp(var.data(), o.var.data(), var.size() * 4) == 0 &&
               std::memcmp(st.data(), o.st.data(), st.size() * 4) == 0 && std::memcmp(og.data(), o.og.data(), og.size() * 4) == 0 && len == o.len && tgt == o.tgt;
    }
    bool Finite() const { return AllFinite(rgb) && AllFinite(var) && AllFinite(st) && AllFinite(og); }
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
    const uint32_t cases = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 240u;
    std::mt19937 rng(20261021u);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    size_t pixels = 0, accepted = 0, moved = 0, padded = 0;
    for (uint32_t t = 0; t < cases; ++t) {
        const uint32_t W = 1 + rng() % (t % 10 == 0 ? 90 : 24), H = 1 + rng() % (t % 10 == 1 ? 70 : 20);
        const uint32_t first = rng() % 3 == 0 ? rng() % H : 0, rows = rng() % 3 == 0 ? 1 + rng() % (H - first) : H - first;
        const uint32_t nshards = 1 + rng() % (t % 7 == 0 ? 12 : 4), block_rows = 1 + rng() % (t % 5 == 0 ? rows + 2 : 4);
        const uint32_t most = rtd::rowset_max_shard_rows(rows, block_rows, nshards);
        const size_t npix = (size_t)W * rows;
        const uint32_t fetch = t % 2 ? RT_TEMPORAL_FETCH_BILINEAR : RT_TEMPORAL_FETCH_NEAREST;
        const rt_variance_params V{RT_VARIANCE_SPATIAL, 1u + t % 3u};
        const Frame cur = RandomFrame(rng, W, rows, t % 4 == 3 ? 2 + rng() % 3 : 1);  // mostly one sample, and then no sq anywhere
        const float* curSq = cur.sq.empty() ? nullptr : cur.sq.data();
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

        // the contiguous twins over the strip itself
        Out want(npix), wantEmpty(npix);
        std::vector<float> wrgb(npix * 3, NAN), wvar(npix, NAN), wst(npix * 4, NAN);
        int rc = rt_unit_temporal_variance_host(cur.hdr.data(), curSq, cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, &Cp, hs.data(), hg.data(),
                                                cur.ids.data(), hl.data(), &P, &T, fetch, &V, want.rgb.data(), want.var.data(), want.st.data(), want.og.data(),
                                                want.len.data(), want.tgt.data());
        CHECK(rc == RT_OK, "case %u, contiguous: rc %d (%s)", t, rc, rtprep::LastError());
        rc = rt_unit_temporal_variance_host(cur.hdr.data(), curSq, cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, &P, &T, fetch, &V, wantEmpty.rgb.data(), wantEmpty.var.data(), wantEmpty.st.data(),
                                            wantEmpty.og.data(), wantEmpty.len.data(), wantEmpty.tgt.data());
        CHECK(rc == RT_OK, "case %u, contiguous, empty history: rc %d (%s)", t, rc, rtprep::LastError());
        rc = rt_unit_denoise_variance_host(cur.hdr.data(), curSq, cur.n, cur.feat.data(), cur.m, W, rows, &P, &V, wrgb.data(), wvar.data(), wst.data());
        CHECK(rc == RT_OK, "case %u, contiguous filter: rc %d (%s)", t, rc, rtprep::LastError());
        CHECK(want.Finite() && wantEmpty.Finite() && AllFinite(wrgb) && AllFinite(wvar) && AllFinite(wst), "case %u: the contiguous twins are not finite", t);

        for (const uint32_t extra : {0u, 1u + (uint32_t)(rng() % 3)}) {
            const uint32_t rows_max = most + extra;
            const Frame parts = CutIntoParts(cur, W, rows, block_rows, nshards, rows_max);
            const float* sq = parts.sq.empty() ? nullptr : parts.sq.data();
            const rt_shard_frame shape = ShapeOf(W, H, first, rows, block_rows, nshards, rows_max, cur.n, cur.m, C);
            Out got(npix), gotEmpty(npix);
            rc = rt_unit_temporal_shards_variance_host(parts.hdr.data(), sq, parts.feat.data(), parts.ids.data(), &shape, &Cp, hs.data(), hg.data(), cur.ids.data(),
                                                       hl.data(), &P, &T, fetch, &V, got.rgb.data(), got.var.data(), got.st.data(), got.og.data(), got.len.data(),
                                                       got.tgt.data());
            CHECK(rc == RT_OK, "case %u, parts: rc %d (%s)", t, rc, rtprep::LastError());
            CHECK(got.SameBytes(want), "case %u (%u x %u rows %u..+%u of %u, %u shards of %u-row blocks, rows_max %u, fetch %u, radius %u): parts != contiguous", t, W,
                  rows, first, rows, H, nshards, block_rows, rows_max, fetch, V.radius);
            rc = rt_unit_temporal_shards_variance_host(parts.hdr.data(), sq, parts.feat.data(), parts.ids.data(), &shape, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       &P, &T, fetch, &V, gotEmpty.rgb.data(), gotEmpty.var.data(), gotEmpty.st.data(), gotEmpty.og.data(),
                                                       gotEmpty.len.data(), gotEmpty.tgt.data());
            CHECK(rc == RT_OK, "case %u, parts, empty history: rc %d (%s)", t, rc, rtprep::LastError());
            CHECK(gotEmpty.SameBytes(wantEmpty), "case %u: parts != contiguous on an empty history", t);
            std::vector<float> rgb(npix * 3, NAN), var(npix, NAN), st(npix * 4, NAN);
            rc = rt_unit_denoise_shards_variance_host(parts.hdr.data(), sq, parts.feat.data(), &shape.parts, &P, &V, rgb.data(), var.data(), st.data());
            CHECK(rc == RT_OK, "case %u, filter over the parts: rc %d (%s)", t, rc, rtprep::LastError());
            CHECK(std::memcmp(rgb.data(), wrgb.data(), npix * 12) == 0 && std::memcmp(var.data(), wvar.data(), npix * 4) == 0 &&
                      std::memcmp(st.data(), wst.data(), npix * 16) == 0,
                  "case %u (%u shards of %u-row blocks, rows_max %u, radius %u): filter over the parts != contiguous filter", t, nshards, block_rows, rows_max,
                  V.radius);
            CHECK(std::memcmp(rgb.data(), gotEmpty.rgb.data(), npix * 12) == 0 && std::memcmp(var.data(), gotEmpty.var.data(), npix * 4) == 0,
                  "case %u: empty history != rt_unit_denoise_shards_variance_host", t);
            if (sq) {  // the moments source through the new twins: the existing twins' bytes
                const rt_variance_params M{RT_VARIANCE_MOMENTS, 99u};
                std::vector<float> a3(npix * 3, NAN), a1(npix, NAN), b3(npix * 3, NAN), b1(npix, NAN);
                rc = rt_unit_denoise_shards_host(parts.hdr.data(), sq, parts.feat.data(), &shape.parts, &P, a3.data(), a1.data());
                const int rc2 = rt_unit_denoise_shards_variance_host(parts.hdr.data(), sq, parts.feat.data(), &shape.parts, &P, &M, b3.data(), b1.data(), nullptr);
                CHECK(rc == RT_OK && rc2 == RT_OK && a3 == b3 && a1 == b1 && AllFinite(a3), "case %u: the moments source differs from rt_unit_denoise_shards_host", t);
                Out o1(npix), o2(npix);
                rc = rt_unit_temporal_shards_host(parts.hdr.data(), sq, parts.feat.data(), parts.ids.data(), &shape, &Cp, hs.data(), hg.data(), cur.ids.data(),
                                                  hl.data(), &P, &T, fetch, o1.rgb.data(), o1.var.data(), o1.st.data(), o1.og.data(), o1.len.data(), o1.tgt.data());
                const int rc3 = rt_unit_temporal_shards_variance_host(parts.hdr.data(), sq, parts.feat.data(), parts.ids.data(), &shape, &Cp, hs.data(), hg.data(),
                                                                      cur.ids.data(), hl.data(), &P, &T, fetch, nullptr, o2.rgb.data(), o2.var.data(), o2.st.data(),
                                                                      o2.og.data(), o2.len.data(), o2.tgt.data());
                CHECK(rc == RT_OK && rc3 == RT_OK && o1.SameBytes(o2), "case %u: vparams == NULL differs from rt_unit_temporal_shards_host", t);
            }
            padded += (size_t)nshards * rows_max * W - npix;
        }
        for (size_t p = 0; p < npix; ++p) {
            CHECK(want.tgt[p] == 0xffffffffu || want.tgt[p] < npix, "case %u pixel %zu: target %u of %zu", t, p, want.tgt[p], npix);
            accepted += want.tgt[p] != 0xffffffffu;
            moved += want.tgt[p] != 0xffffffffu && want.tgt[p] != p;
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
        const Frame s = RandomFrame(rng, W, rows, 2);
        const Frame f = CutIntoParts(s, W, rows, 1, nshards, rows_max);
        const float from[3] = {3.f, 1.f, 4.f};
        const rt_camera C = LookAtOrigin(from, 0.5f, 0.4f);
        std::vector<float> hs(npix * 4, 0.f), hg(npix * 8, 0.f), rgb(npix * 3), var(npix);
        std::vector<uint32_t> hl(npix, 1u), hid(npix, 1u);
        const rt_shard_frame good = ShapeOf(W, H, first, rows, 1, nshards, rows_max, 1, 1, C);
        const rt_variance_params S1{RT_VARIANCE_SPATIAL, 1};
        auto plain = [&](const rt_shard_frame& sh, const float* sq, const rt_variance_params* V) {
            return rt_unit_denoise_shards_variance_host(f.hdr.data(), sq, f.feat.data(), &sh.parts, nullptr, V, rgb.data(), var.data(), nullptr);
        };
        auto temporal = [&](const rt_shard_frame& sh, const float* sq, const rt_variance_params* V, uint32_t fetch) {
            return rt_unit_temporal_shards_variance_host(f.hdr.data(), sq, f.feat.data(), f.ids.data(), &sh, &C, hs.data(), hg.data(), hid.data(), hl.data(), nullptr,
                                                         nullptr, fetch, V, rgb.data(), var.data(), nullptr, nullptr, nullptr, nullptr);
        };
        CHECK(plain(good, nullptr, &S1) == RT_OK, "spatial, n = 1, no sq: %s", rtprep::LastError());
        CHECK(temporal(good, nullptr, &S1, 1) == RT_OK && temporal(good, nullptr, &S1, 4) == RT_OK, "spatial temporal, n = 1, no sq: %s", rtprep::LastError());
        for (const uint32_t r : {0u, 4u, 0xffffffffu}) {
            const rt_variance_params V{RT_VARIANCE_SPATIAL, r};
            CHECK(plain(good, nullptr, &V) == RT_ERR_INVALID_ARG && temporal(good, nullptr, &V, 4) == RT_ERR_INVALID_ARG, "radius %u", r);
        }
        for (const uint32_t src : {2u, 0xffffffffu}) {
            const rt_variance_params V{src, 1};
            CHECK(plain(good, f.sq.data(), &V) == RT_ERR_INVALID_ARG && temporal(good, f.sq.data(), &V, 4) == RT_ERR_INVALID_ARG, "source %u", src);
        }
        rt_shard_frame sh = good;
        sh.parts.n = 0;
        CHECK(plain(sh, nullptr, &S1) == RT_ERR_SEQUENCE && temporal(sh, nullptr, &S1, 4) == RT_ERR_SEQUENCE, "n == 0 under the spatial source");
        sh = good, sh.parts.m = 0;
        CHECK(plain(sh, nullptr, &S1) == RT_ERR_SEQUENCE && temporal(sh, nullptr, &S1, 4) == RT_ERR_SEQUENCE, "m == 0");
        const rt_variance_params M{RT_VARIANCE_MOMENTS, 0};
        for (const rt_variance_params* V : {(const rt_variance_params*)nullptr, &M}) {
            CHECK(plain(good, f.sq.data(), V) == RT_ERR_SEQUENCE && temporal(good, f.sq.data(), V, 4) == RT_ERR_SEQUENCE, "n == 1 under the moments source");
            sh = good, sh.parts.n = 2;
            CHECK(plain(sh, f.sq.data(), V) == RT_OK && temporal(sh, f.sq.data(), V, 4) == RT_OK, "the moments source: %s", rtprep::LastError());
            CHECK(plain(sh, nullptr, V) == RT_ERR_INVALID_ARG && temporal(sh, nullptr, V, 4) == RT_ERR_INVALID_ARG, "no sq under the moments source");
        }
        for (uint32_t bad : {0u, 2u, 5u}) CHECK(temporal(good, nullptr, &S1, bad) == RT_ERR_INVALID_ARG, "fetch %u", bad);
        sh = good, sh.parts.W = 0;
        CHECK(plain(sh, nullptr, &S1) == RT_ERR_INVALID_ARG && temporal(sh, nullptr, &S1, 4) == RT_ERR_INVALID_ARG, "W == 0");
        sh = good, sh.parts.rs.nshards = 0;
        CHECK(plain(sh, nullptr, &S1) == RT_ERR_INVALID_ARG && temporal(sh, nullptr, &S1, 4) == RT_ERR_INVALID_ARG, "no shards");
        sh = good, sh.parts.rows_max = rows_max - 1;
        CHECK(plain(sh, nullptr, &S1) == RT_ERR_INVALID_ARG && temporal(sh, nullptr, &S1, 4) == RT_ERR_INVALID_ARG, "rows_max below the largest shard");
        sh = good, sh.H = first + rows - 1;
        CHECK(temporal(sh, nullptr, &S1, 4) == RT_ERR_INVALID_ARG, "rows beyond the image");
    }
    if (g_fail) {
        std::fprintf(stderr, "denoise_shards_spatial_selftest: %d failures\n", g_fail);
        return 1;
    }
    std::printf("denoise_shards_spatial_selftest ok: %u cases, %zu pixels, %zu accepted (%zu of them elsewhere), %zu padding pixels\n", cases, pixels, accepted, moved,
                padded);
    return 0;
}
