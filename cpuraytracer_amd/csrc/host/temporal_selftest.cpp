// temporal_selftest.cpp -- the temporal twin (rt_temporal_host.cpp over ../rt_temporal.h) in a program of its own: random strips,
// histories and pairs of cameras with invariants no frame should break.  No HIP, no librt_hip.so; also built under ASan + UBSan
// (Makefile temporal_selftest_san), where every index the gather forms is checked: the history's arrays are exactly npix long.
//   - len within 1 .. max_history, target in range or 0xffffffff, len == 1 wherever target == 0xffffffff;
//   - an accepted pixel's history pixel has len >= 1, and len' == min(lenh, max_history - 1) + 1;
//   - finite in -> finite state out, v' >= 0;
//   - an empty history gives rt_unit_denoise_host's bits and len == 1 everywhere;
//   - cameras that look away, NaN and infinite camera records reject without reading;
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
#include "../rt_temporal.h"
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

static Frame RandomFrame(std::mt19937& rng, size_t npix) {
    Frame s;
    s.n = 2 + rng() % 6;
    s.m = 1 + rng() % 4;
    s.hdr.resize(npix * 3);
    s.sq.resize(npix * 3);
    s.feat.resize(npix * 8);
    s.ids.resize(npix);
    std::uniform_real_distribution<float> u(0.f, 1.f);
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
        const bool sky = rng() % 4 == 0;
        const float fm = (float)s.m;
        float* f = &s.feat[8 * p];
        for (int c = 0; c < 3; ++c) f[c] = u(rng) * fm;
        for (int c = 3; c < 6; ++c) f[c] = sky ? 0.f : (0.2f * u(rng) - 0.1f) * fm;
        f[7] = sky ? 0.f : (float)(1 + rng() % s.m);
        f[6] = sky ? 0.f : (2.f + 30.f * u(rng)) * f[7];
        s.ids[p] = sky ? 0xffffffffu : rng() % 3;
    }
    return s;
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

int main(int argc, char** argv) {
    const uint32_t cases = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 400u;
    std::mt19937 rng(20261020u);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    rt_temporal_params def;
    CHECK(rt_temporal_default_params(&def) == RT_OK && def.max_history == 2 && def.use_id == 1 && def.depth_tol == 0.1f && def.normal_tol == 0.1f &&
              def.coverage_tol == 0.25f,
          "defaults");
    CHECK(rt_temporal_default_params(nullptr) == RT_ERR_INVALID_ARG, "null defaults");
    size_t pixels = 0, accepted = 0;
    for (uint32_t t = 0; t < cases; ++t) {
        const uint32_t W = 1 + rng() % (t % 10 == 0 ? 90 : 24), H = 1 + rng() % (t % 10 == 1 ? 70 : 20);
        const uint32_t first = rng() % 3 == 0 ? rng() % H : 0, rows = rng() % 3 == 0 ? 1 + rng() % (H - first) : H - first;
        const size_t npix = (size_t)W * rows;
        const Frame cur = RandomFrame(rng, npix), old = RandomFrame(rng, npix);
        // the history: the guides of `old`, a random state and random lengths (0 = a pixel that holds nothing)
        rt_temporal_params T = def;
        T.max_history = 1 + rng() % 64;
        T.use_id = rng() % 2;
        if (t % 4 == 1) T.depth_tol = 10.f * u(rng), T.normal_tol = 4.f * u(rng), T.coverage_tol = u(rng);
        if (t % 4 == 2) T.depth_tol = 3.0e38f, T.normal_tol = 3.0e38f, T.coverage_tol = 3.0e38f;
        std::vector<float> hs(npix * 4), hg(npix * 8);
        std::vector<uint32_t> hl(npix);
        for (size_t p = 0; p < npix; ++p) {
            for (int k = 0; k < 4; ++k) hs[4 * p + k] = 2.f * u(rng);
            for (int k = 0; k < 8; ++k) hg[8 * p + k] = old.feat[8 * p + k] / (float)old.m;
            hl[p] = rng() % 70;
        }
        const float from[3] = {20.f * u(rng) - 10.f, 6.f * u(rng) - 1.f, 20.f * u(rng) - 10.f};
        float from2[3];
        const uint32_t move = t % 5;  // 0 the same camera, 1 a small move, 2 anywhere, 3 turned 180 degrees where it stands, 4 a broken record
        for (int k = 0; k < 3; ++k) from2[k] = move == 0 || move == 3 ? from[k] : (move == 1 ? from[k] + 0.2f * u(rng) - 0.1f : 20.f * u(rng) - 10.f);
        const float hw = 0.2f + u(rng), hh = hw * (float)H / (float)W;
        const rt_camera C = LookAtOrigin(from, hw, hh);
        rt_camera Cp = LookAtOrigin(from2, hw, hh);
        if (move == 3)
            for (int k = 0; k < 3; ++k) Cp.origin_image_plane[k] = Cp.origin[k] - (Cp.origin_image_plane[k] - Cp.origin[k]);
        if (move == 4) {
            const float bad[4] = {NAN, INFINITY, -INFINITY, 0.f};
            float* field = rng() % 2 ? Cp.x : (rng() % 2 ? Cp.origin : Cp.origin_image_plane);
            field[rng() % 3] = bad[rng() % 4];
        }
        rt_denoise_params P;
        rt_denoise_default_params(&P);
        P.levels = 1 + rng() % 3;
        std::vector<float> rgb(npix * 3, NAN), var(npix, NAN), st(npix * 4, NAN), og(npix * 8, NAN);
        std::vector<uint32_t> len(npix, 12345u), tgt(npix, 12345u);
        int rc = rt_unit_temporal_host(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, &Cp, hs.data(),
                                       hg.data(), old.ids.data(), hl.data(), &P, &T, rgb.data(), var.data(), st.data(), og.data(), len.data(), tgt.data());
        CHECK(rc == RT_OK, "case %u: rc %d (%s)", t, rc, rtprep::LastError());
        for (size_t p = 0; p < npix; ++p) {
            CHECK(len[p] >= 1 && len[p] <= T.max_history, "case %u pixel %zu: len %u of %u", t, p, len[p], T.max_history);
            CHECK(tgt[p] == 0xffffffffu || tgt[p] < npix, "case %u pixel %zu: target %u of %zu", t, p, tgt[p], npix);
            if (tgt[p] == 0xffffffffu) {
                CHECK(len[p] == 1, "case %u pixel %zu: rejected with len %u", t, p, len[p]);
            } else {
                const uint32_t lh = hl[tgt[p]], cap = T.max_history - 1u;
                CHECK(lh >= 1 && len[p] == (lh < cap ? lh : cap) + 1u, "case %u pixel %zu: len %u from %u", t, p, len[p], lh);
                CHECK(!T.use_id || cur.ids[p] == old.ids[tgt[p]], "case %u pixel %zu: ids differ", t, p);
                ++accepted;
            }
            for (int k = 0; k < 4; ++k) CHECK(std::isfinite(st[4 * p + k]), "case %u pixel %zu: state %d", t, p, k);
            CHECK(st[4 * p + 3] >= 0.f && var[p] >= 0.f && std::isfinite(var[p]), "case %u pixel %zu: variance", t, p);
            CHECK(move != 3 || tgt[p] == 0xffffffffu, "case %u pixel %zu: accepted behind the camera", t, p);
        }
        pixels += npix;
        // an empty history: the filter alone
        std::vector<float> rgb0(npix * 3, NAN), var0(npix, NAN), rgb1(npix * 3, NAN), var1(npix, NAN);
        rc = rt_unit_temporal_host(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, &P, &T, rgb0.data(), var0.data(), nullptr, nullptr, len.data(), tgt.data());
        CHECK(rc == RT_OK, "case %u, empty history: rc %d (%s)", t, rc, rtprep::LastError());
        rc = rt_unit_denoise_host(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, W, rows, &P, rgb1.data(), var1.data());
        CHECK(rc == RT_OK, "case %u, filter: rc %d", t, rc);
        CHECK(std::memcmp(rgb0.data(), rgb1.data(), npix * 12) == 0 && std::memcmp(var0.data(), var1.data(), npix * 4) == 0, "case %u: empty history != filter", t);
        for (size_t p = 0; p < npix; ++p) CHECK(len[p] == 1 && tgt[p] == 0xffffffffu, "case %u pixel %zu: empty history blended", t, p);
    }
    CHECK(accepted > pixels / 50, "only %zu of %zu pixels were ever accepted: the cases do not exercise the blend", accepted, pixels);

    // refusals
    {
        const size_t npix = 12;
        const Frame f = RandomFrame(rng, npix);
        const float from[3] = {3.f, 1.f, 4.f};
        const rt_camera C = LookAtOrigin(from, 0.5f, 0.4f);
        std::vector<float> hs(npix * 4, 0.f), hg(npix * 8, 0.f), rgb(npix * 3), var(npix);
        std::vector<uint32_t> hl(npix, 1u);
        auto call = [&](uint32_t n, uint32_t m, uint32_t W, uint32_t H, uint32_t first, uint32_t rows, const rt_camera* cp, const rt_temporal_params* T) {
            return rt_unit_temporal_host(f.hdr.data(), f.sq.data(), n, f.feat.data(), m, f.ids.data(), W, H, first, rows, &C, cp, hs.data(), hg.data(),
                                         f.ids.data(), hl.data(), nullptr, T, rgb.data(), var.data(), nullptr, nullptr, nullptr, nullptr);
        };
        CHECK(call(2, 1, 4, 3, 0, 3, &C, nullptr) == RT_OK, "the plain call: %s", rtprep::LastError());
        CHECK(call(1, 1, 4, 3, 0, 3, &C, nullptr) == RT_ERR_SEQUENCE, "n < 2");
        CHECK(call(2, 0, 4, 3, 0, 3, &C, nullptr) == RT_ERR_SEQUENCE, "m == 0");
        CHECK(call(2, 1, 0, 3, 0, 3, &C, nullptr) == RT_ERR_INVALID_ARG, "W == 0");
        CHECK(call(2, 1, 4, 3, 1, 3, &C, nullptr) == RT_ERR_INVALID_ARG, "rows beyond the image");
        CHECK(call(2, 1, 4, 3, 0, 0, &C, nullptr) == RT_ERR_INVALID_ARG, "no rows");
        CHECK(call(2, 1, 4, 3, 0, 3, nullptr, nullptr) == RT_ERR_INVALID_ARG, "a history without its camera");
        rt_temporal_params T = def;
        T.max_history = 0;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T) == RT_ERR_INVALID_ARG, "max_history 0");
        T.max_history = 65;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T) == RT_ERR_INVALID_ARG, "max_history 65");
        T = def;
        T.depth_tol = -1.f;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T) == RT_ERR_INVALID_ARG, "negative tolerance");
        T = def;
        T.normal_tol = NAN;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T) == RT_ERR_INVALID_ARG, "NaN tolerance");
        T = def;
        T.coverage_tol = INFINITY;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T) == RT_ERR_INVALID_ARG, "infinite tolerance");
    }
    if (g_fail) {
        std::fprintf(stderr, "temporal_selftest: %d failures\n", g_fail);
        return 1;
    }
    std::printf("temporal_selftest ok: %u cases, %zu pixels, %zu accepted\n", cases, pixels, accepted);
    return 0;
}
