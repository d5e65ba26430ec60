// temporal_bilinear_selftest.cpp -- the temporal twin's bilinear fetch (rt_unit_temporal_host_fetch, rt_temporal_host.cpp over
// ../rt_temporal.h) in a program of its own: random strips, histories and pairs of cameras.  No HIP, no librt_hip.so; also built under
// ASan + UBSan (Makefile temporal_bilinear_selftest_san), where every index the gather forms is checked: the history's arrays are exactly
// npix long.  The taps of every pixel are formed here a second time from the reprojected point, and against them:
//   - every tap that is inside by its column and row has an index below npix, and a tap outside is never the target;
//   - the weights of the participating taps sum to sw in (0, 1 + 2^-20] wherever the pixel is accepted;
//   - target names a participating tap of the greatest weight, the first of them; no participating tap: target 0xffffffff, len 1;
//   - len' == min(shortest participating length, max_history - 1) + 1 <= max_history;
//   - finite in -> finite state out, v' >= 0, and a colour between the participating taps' extremes and the current pixel's;
//   - fetch 1 through the new entry gives rt_unit_temporal_host's bytes; an empty history gives rt_unit_denoise_host's;
//   - the defaults and the refusals.
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

// smooth: guides and ids that vary slowly over the strip, so that most taps pass the validation
static Frame RandomFrame(std::mt19937& rng, uint32_t W, uint32_t rows, bool smooth) {
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
        const bool sky = smooth ? (p % W) >= cut : rng() % 4 == 0;
        const float fm = (float)s.m;
        float* f = &s.feat[8 * p];
        for (int c = 0; c < 3; ++c) f[c] = u(rng) * fm;
        for (int c = 3; c < 6; ++c) f[c] = sky ? 0.f : (0.2f * u(rng) - 0.1f) * fm;
        f[7] = sky ? 0.f : (smooth ? fm : (float)(1 + rng() % s.m));
        f[6] = sky ? 0.f : (smooth ? 12.f + 0.05f * u(rng) : 2.f + 30.f * u(rng)) * f[7];
        s.ids[p] = sky ? 0xffffffffu : (smooth ? 1u : rng() % 3);
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
    std::mt19937 rng(20261021u);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    rt_temporal_params def, def1, def4;
    CHECK(rt_temporal_default_params(&def) == RT_OK, "defaults");
    CHECK(rt_temporal_default_params_fetch(RT_TEMPORAL_FETCH_NEAREST, &def1) == RT_OK && std::memcmp(&def, &def1, sizeof def) == 0, "fetch 1 defaults");
    CHECK(rt_temporal_default_params_fetch(RT_TEMPORAL_FETCH_BILINEAR, &def4) == RT_OK && def4.max_history == 3 && def4.use_id == def.use_id &&
              def4.depth_tol == def.depth_tol && def4.normal_tol == def.normal_tol && def4.coverage_tol == def.coverage_tol,
          "fetch 4 defaults");
    for (uint32_t bad : {0u, 2u, 3u, 5u, 0xffffffffu}) CHECK(rt_temporal_default_params_fetch(bad, &def1) == RT_ERR_INVALID_ARG, "defaults of fetch %u", bad);
    CHECK(rt_temporal_default_params_fetch(RT_TEMPORAL_FETCH_BILINEAR, nullptr) == RT_ERR_INVALID_ARG, "null defaults");

    size_t pixels = 0, accepted = 0, partial = 0, full = 0;
    for (uint32_t t = 0; t < cases; ++t) {
        const uint32_t W = 1 + rng() % (t % 10 == 0 ? 90 : 24), H = 1 + rng() % (t % 10 == 1 ? 70 : 20);
        const uint32_t first = rng() % 3 == 0 ? rng() % H : 0, rows = rng() % 3 == 0 ? 1 + rng() % (H - first) : H - first;
        const size_t npix = (size_t)W * rows;
        const bool smooth = t % 2 == 0;
        const Frame cur = RandomFrame(rng, W, rows, smooth);
        Frame old = smooth ? cur : RandomFrame(rng, W, rows, false);
        rt_temporal_params T = def4;
        T.max_history = 1 + rng() % 64;
        T.use_id = rng() % 2;
        if (t % 4 == 1) T.depth_tol = 10.f * u(rng), T.normal_tol = 4.f * u(rng), T.coverage_tol = u(rng);
        if (t % 4 == 2) T.depth_tol = 3.0e38f, T.normal_tol = 3.0e38f, T.coverage_tol = 3.0e38f;
        if (smooth) T.depth_tol = 0.9f;
        std::vector<float> hs(npix * 4), hg(npix * 8);
        std::vector<uint32_t> hl(npix);
        for (size_t p = 0; p < npix; ++p) {
            for (int k = 0; k < 4; ++k) hs[4 * p + k] = 2.f * u(rng);
            for (int k = 0; k < 8; ++k) hg[8 * p + k] = old.feat[8 * p + k] / (float)old.m;
            hl[p] = smooth && rng() % 8 ? 1 + rng() % 69 : rng() % 70;  // 0: a pixel that holds nothing
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
        int rc = rt_unit_temporal_host_fetch(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, &Cp, hs.data(),
                                             hg.data(), old.ids.data(), hl.data(), &P, &T, RT_TEMPORAL_FETCH_BILINEAR, rgb.data(), var.data(), st.data(),
                                             og.data(), len.data(), tgt.data());
        CHECK(rc == RT_OK, "case %u: rc %d (%s)", t, rc, rtprep::LastError());
        const rtd::TemporalGeom G{W, H, first, rows};
        const rtd::TemporalCam tc = rtdn::CamOf(C), tcp = rtdn::CamOf(Cp);
        const rtd::TemporalParams TT{T.max_history, T.use_id, T.depth_tol, T.normal_tol, T.coverage_tol};
        for (size_t p = 0; p < npix; ++p) {
            const uint32_t x = (uint32_t)(p % W), ly = (uint32_t)(p / W);
            CHECK(len[p] >= 1 && len[p] <= T.max_history, "case %u pixel %zu: len %u of %u", t, p, len[p], T.max_history);
            for (int k = 0; k < 4; ++k) CHECK(std::isfinite(st[4 * p + k]), "case %u pixel %zu: state %d", t, p, k);
            CHECK(st[4 * p + 3] >= 0.f && var[p] >= 0.f && std::isfinite(var[p]), "case %u pixel %zu: variance", t, p);
            CHECK(move != 3 || tgt[p] == 0xffffffffu, "case %u pixel %zu: accepted behind the camera", t, p);
            // the taps, a second time
            float fx = 0.f, fy = 0.f, dist = 0.f;
            uint32_t xi = 0, yi = 0, want = 0xffffffffu, lmin = 0xffffffffu, taking = 0;
            float sw = 0.f, wbest = 0.f, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            if (rtd::temporal_reproject_point(G, tc, tcp, x, first + ly, &og[8 * p], fx, fy, xi, yi, dist)) {
                CHECK(xi < W && yi >= first && yi < first + rows, "case %u pixel %zu: (%u, %u) outside", t, p, xi, yi);
                rtd::TemporalTaps B;
                rtd::temporal_taps(fx, fy, xi, yi, B);
                CHECK(B.tx >= 0.f && B.tx <= 1.f && B.ty >= 0.f && B.ty <= 1.f, "case %u pixel %zu: t (%g, %g)", t, p, B.tx, B.ty);
                CHECK((B.x0 == (int32_t)xi || B.x0 == (int32_t)xi - 1) && (B.y0 == (int32_t)yi || B.y0 == (int32_t)yi - 1), "case %u pixel %zu: tap (0, 0)", t, p);
                // the point lies between the centres of the taps
                CHECK((float)B.x0 + 0.5f <= fx && fx <= (float)B.x0 + 1.5f && (float)B.y0 + 0.5f <= fy && fy <= (float)B.y0 + 1.5f, "case %u pixel %zu: centres", t, p);
                for (int k = 0; k < 4; ++k) {
                    const int64_t qx = (int64_t)B.x0 + (k & 1), qy = (int64_t)B.y0 + (k >> 1);
                    const bool inside = qx >= 0 && qx < (int64_t)W && qy >= (int64_t)first && qy < (int64_t)first + rows;
                    uint32_t q = 0xdeadbeefu;
                    const bool in = rtd::temporal_tap_index(G, B, k, q);
                    CHECK(in == inside, "case %u pixel %zu tap %d: inside %d, temporal_tap_index %d", t, p, k, (int)inside, (int)in);
                    if (!in) continue;
                    CHECK(q < npix && q == (uint64_t)(qy - first) * W + (uint64_t)qx, "case %u pixel %zu tap %d: index %u of %zu", t, p, k, q, npix);
                    const float w = rtd::temporal_tap_weight(B, k);
                    CHECK(w >= 0.f && w <= 1.f, "case %u pixel %zu tap %d: weight %g", t, p, k, w);
                    if (!(w > 0.f) || !rtd::temporal_validate(TT, &og[8 * p], cur.ids[p], dist, &hg[8 * (size_t)q], old.ids[q], hl[q])) continue;
                    ++taking;
                    sw += w;
                    lmin = hl[q] < lmin ? hl[q] : lmin;
                    if (w > wbest) wbest = w, want = q;
                    for (int c = 0; c < 3; ++c) {
                        lo[c] = std::fmin(lo[c], hs[4 * (size_t)q + c]);
                        hi[c] = std::fmax(hi[c], hs[4 * (size_t)q + c]);
                    }
                }
            }
            CHECK(tgt[p] == want, "case %u pixel %zu: target %u, the greatest participating tap is %u", t, p, tgt[p], want);
            if (taking == 0) {
                CHECK(tgt[p] == 0xffffffffu && len[p] == 1, "case %u pixel %zu: no tap took part, len %u", t, p, len[p]);
                continue;
            }
            ++accepted;
            if (taking == 4) ++full; else ++partial;
            CHECK(sw > 0.f && sw <= 1.f + 9.5367431640625e-07f, "case %u pixel %zu: sw %.9g", t, p, sw);
            const uint32_t cap = T.max_history - 1u;
            CHECK(lmin >= 1 && len[p] == (lmin < cap ? lmin : cap) + 1u, "case %u pixel %zu: len %u from %u", t, p, len[p], lmin);
            // the blend is a convex combination of the current colour and a weighted mean of the participating taps
            for (int c = 0; c < 3; ++c) {
                const float cc = cur.hdr[3 * p + c] / (float)cur.n;
                const float l = std::fmin(lo[c], cc), h = std::fmax(hi[c], cc), eps = 1e-5f * (std::fabs(l) + std::fabs(h) + 1.f);
                CHECK(st[4 * p + c] >= l - eps && st[4 * p + c] <= h + eps, "case %u pixel %zu: colour %d = %g outside [%g, %g]", t, p, c, st[4 * p + c], l, h);
            }
        }
        pixels += npix;
        // fetch 1 through the new entry: the old entry's bytes
        std::vector<float> rgbA(npix * 3, NAN), varA(npix, NAN), stA(npix * 4, NAN), rgbB(npix * 3, NAN), varB(npix, NAN), stB(npix * 4, NAN);
        std::vector<uint32_t> lenA(npix), tgtA(npix), lenB(npix), tgtB(npix);
        rc = rt_unit_temporal_host_fetch(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, &Cp, hs.data(),
                                         hg.data(), old.ids.data(), hl.data(), &P, &T, RT_TEMPORAL_FETCH_NEAREST, rgbA.data(), varA.data(), stA.data(), nullptr,
                                         lenA.data(), tgtA.data());
        CHECK(rc == RT_OK, "case %u, fetch 1: rc %d (%s)", t, rc, rtprep::LastError());
        rc = rt_unit_temporal_host(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, &Cp, hs.data(), hg.data(),
                                   old.ids.data(), hl.data(), &P, &T, rgbB.data(), varB.data(), stB.data(), nullptr, lenB.data(), tgtB.data());
        CHECK(rc == RT_OK, "case %u, the old entry: rc %d (%s)", t, rc, rtprep::LastError());
        CHECK(std::memcmp(rgbA.data(), rgbB.data(), npix * 12) == 0 && std::memcmp(varA.data(), varB.data(), npix * 4) == 0 &&
                  std::memcmp(stA.data(), stB.data(), npix * 16) == 0 && lenA == lenB && tgtA == tgtB,
              "case %u: fetch 1 != rt_unit_temporal_host", t);
        // an empty history: the filter alone
        rc = rt_unit_temporal_host_fetch(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, cur.ids.data(), W, H, first, rows, &C, nullptr, nullptr,
                                         nullptr, nullptr, nullptr, &P, &T, RT_TEMPORAL_FETCH_BILINEAR, rgbA.data(), varA.data(), nullptr, nullptr, lenA.data(),
                                         tgtA.data());
        CHECK(rc == RT_OK, "case %u, empty history: rc %d (%s)", t, rc, rtprep::LastError());
        rc = rt_unit_denoise_host(cur.hdr.data(), cur.sq.data(), cur.n, cur.feat.data(), cur.m, W, rows, &P, rgbB.data(), varB.data());
        CHECK(rc == RT_OK, "case %u, filter: rc %d", t, rc);
        CHECK(std::memcmp(rgbA.data(), rgbB.data(), npix * 12) == 0 && std::memcmp(varA.data(), varB.data(), npix * 4) == 0, "case %u: empty history != filter", t);
        for (size_t p = 0; p < npix; ++p) CHECK(lenA[p] == 1 && tgtA[p] == 0xffffffffu, "case %u pixel %zu: empty history blended", t, p);
    }
    CHECK(accepted > pixels / 20, "only %zu of %zu pixels were ever accepted: the cases do not exercise the blend", accepted, pixels);
    CHECK(full > pixels / 50 && partial > pixels / 50, "%zu pixels with four taps, %zu with fewer, of %zu: the cases do not exercise both", full, partial, pixels);

    // refusals
    {
        const uint32_t W = 4, rows = 3;
        const size_t npix = (size_t)W * rows;
        const Frame f = RandomFrame(rng, W, rows, false);
        const float from[3] = {3.f, 1.f, 4.f};
        const rt_camera C = LookAtOrigin(from, 0.5f, 0.4f);
        std::vector<float> hs(npix * 4, 0.f), hg(npix * 8, 0.f), rgb(npix * 3), var(npix);
        std::vector<uint32_t> hl(npix, 1u);
        auto call = [&](uint32_t n, uint32_t m, uint32_t w, uint32_t h, uint32_t first, uint32_t nrows, const rt_camera* cp, const rt_temporal_params* T, uint32_t fetch) {
            return rt_unit_temporal_host_fetch(f.hdr.data(), f.sq.data(), n, f.feat.data(), m, f.ids.data(), w, h, first, nrows, &C, cp, hs.data(), hg.data(),
                                               f.ids.data(), hl.data(), nullptr, T, fetch, rgb.data(), var.data(), nullptr, nullptr, nullptr, nullptr);
        };
        CHECK(call(2, 1, 4, 3, 0, 3, &C, nullptr, 4) == RT_OK, "the plain call: %s", rtprep::LastError());
        CHECK(call(2, 1, 4, 3, 0, 3, &C, nullptr, 1) == RT_OK, "the plain call, fetch 1: %s", rtprep::LastError());
        for (uint32_t bad : {0u, 2u, 3u, 5u, 0xffffffffu}) CHECK(call(2, 1, 4, 3, 0, 3, &C, nullptr, bad) == RT_ERR_INVALID_ARG, "fetch %u", bad);
        CHECK(call(1, 1, 4, 3, 0, 3, &C, nullptr, 4) == RT_ERR_SEQUENCE, "n < 2");
        CHECK(call(2, 0, 4, 3, 0, 3, &C, nullptr, 4) == RT_ERR_SEQUENCE, "m == 0");
        CHECK(call(2, 1, 0, 3, 0, 3, &C, nullptr, 4) == RT_ERR_INVALID_ARG, "W == 0");
        CHECK(call(2, 1, 4, 3, 1, 3, &C, nullptr, 4) == RT_ERR_INVALID_ARG, "rows beyond the image");
        CHECK(call(2, 1, 4, 3, 0, 0, &C, nullptr, 4) == RT_ERR_INVALID_ARG, "no rows");
        CHECK(call(2, 1, 4, 3, 0, 3, nullptr, nullptr, 4) == RT_ERR_INVALID_ARG, "a history without its camera");
        rt_temporal_params T = def4;
        T.max_history = 0;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T, 4) == RT_ERR_INVALID_ARG, "max_history 0");
        T.max_history = 65;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T, 4) == RT_ERR_INVALID_ARG, "max_history 65");
        T = def4;
        T.depth_tol = -1.f;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T, 4) == RT_ERR_INVALID_ARG, "negative tolerance");
        T = def4;
        T.normal_tol = NAN;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T, 4) == RT_ERR_INVALID_ARG, "NaN tolerance");
        T = def4;
        T.coverage_tol = INFINITY;
        CHECK(call(2, 1, 4, 3, 0, 3, &C, &T, 4) == RT_ERR_INVALID_ARG, "infinite tolerance");
    }
    if (g_fail) {
        std::fprintf(stderr, "temporal_bilinear_selftest: %d failures\n", g_fail);
        return 1;
    }
    std::printf("temporal_bilinear_selftest ok: %u cases, %zu pixels, %zu accepted (%zu with four taps, %zu with fewer)\n", cases, pixels, accepted, full, partial);
    return 0;
}
