// denoise_spatial_selftest.cpp -- the spatial variance source of the host twins (rt_unit_denoise_variance_host, rt_denoise_host.cpp, and
// rt_unit_temporal_variance_host, rt_temporal_host.cpp, over ../rt_denoise.h) in a program of its own: random strips, radii, ragged
// shapes and row bands with invariants no picture should break.  No HIP, no librt_hip.so; also built under ASan + UBSan (Makefile
// denoise_spatial_selftest_san), where every index the window forms is checked: the buffers end with the strip, and sq is a null pointer.
//   - the prepared state is (hdr / n, v0) with v0 finite and >= 0, at n = 1 as at any n, whatever the feature sample count m;
//   - v0 is a weighted variance: per channel it stays below the squared range of c0 over the pixel's window (plus rounding);
//   - it is formed a second time here, tap by tap in double precision, and agrees to rounding;
//   - a constant picture of power-of-two values has v0 == 0 exactly, whatever the guides (every product and sum is then exact);
//   - the moments source gives rt_unit_denoise_host's bits;
//   - the temporal twin on an empty history over a band of rows (first_row > 0) leaves the same prepared state and the same den;
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
#include "../rt_denoise.h"
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

struct Strips {
    uint32_t W, rows, n, m;
    std::vector<float> hdr, feat;
    std::vector<uint32_t> ids;
};

static Strips RandomStrips(std::mt19937& rng, uint32_t W, uint32_t rows) {
    Strips s;
    s.W = W;
    s.rows = rows;
    s.n = rng() % 3 == 0 ? 1u : 1u + rng() % 8;
    s.m = 1 + rng() % 8;
    const size_t npix = (size_t)W * rows;
    s.hdr.resize(npix * 3);
    s.feat.resize(npix * 8);
    s.ids.resize(npix);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    for (size_t p = 0; p < npix; ++p) {
        const uint32_t kind = rng() % 8;  // 0 black, 1 a constant, else noisy
        for (int c = 0; c < 3; ++c) s.hdr[3 * p + c] = kind == 0 ? 0.f : (kind == 1 ? 0.5f * (float)s.n : 4.f * u(rng) * u(rng) * (float)s.n);
        const bool sky = rng() % 4 == 0;
        const uint32_t band = (uint32_t)((p % W) / 3) % 4;  // objects as vertical bands: neighbours often share guides and often do not
        const float fm = (float)s.m;
        float* f = &s.feat[8 * p];
        for (int c = 0; c < 3; ++c) f[c] = (0.25f * (float)band + 0.1f * u(rng)) * fm;
        for (int c = 3; c < 6; ++c) f[c] = sky ? 0.f : ((c - 3 == (int)band % 3 ? 1.f : 0.f) + 0.02f * u(rng)) * fm;
        f[6] = sky ? 0.f : (5.f + 3.f * (float)band + 0.05f * u(rng)) * fm;
        f[7] = sky ? 0.f : (float)(1 + rng() % s.m);
        s.ids[p] = sky ? 0xffffffffu : band;
    }
    return s;
}

// v0 of pixel (x, y) a second time: the contract's taps in double precision over the twin's own c0 and g
static double SecondV0(const Strips& s, const std::vector<float>& c0, const std::vector<float>& g, const rt_denoise_params& P, int R, int x, int y, double range2[3]) {
    double s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0}, sw = 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const float* gp = &g[8 * ((size_t)y * s.W + x)];
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)s.W || qy >= (int)s.rows) continue;
            const size_t q = (size_t)qy * s.W + qx;
            const float* gq = &g[8 * q];
            double dn = 0, da = 0;
            for (int k = 0; k < 3; ++k) dn += ((double)gp[3 + k] - gq[3 + k]) * ((double)gp[3 + k] - gq[3 + k]), da += ((double)gp[k] - gq[k]) * ((double)gp[k] - gq[k]);
            const double dz = (double)gp[6] - gq[6], zm = gp[6] > gq[6] ? gp[6] : gq[6], dc = (double)gp[7] - gq[7];
            const double xx = P.k_normal * dn + P.k_depth * (dz * dz / (zm * zm + 1e-12)) + P.k_albedo * da + P.k_coverage * dc * dc;
            const double w = 1.0 / (1.0 + xx);
            for (int k = 0; k < 3; ++k) {
                const double c = c0[4 * q + k];
                s1[k] += w * c, s2[k] += w * c * c;
                lo[k] = c < lo[k] ? c : lo[k], hi[k] = c > hi[k] ? c : hi[k];
            }
            sw += w;
        }
    double v = 0;
    for (int k = 0; k < 3; ++k) {
        const double mu = s1[k] / sw, d = s2[k] / sw - mu * mu;
        v += d > 0 ? d : 0;
        range2[k] = (hi[k] - lo[k]) * (hi[k] - lo[k]);
    }
    return v;
}

int main(int argc, char** argv) {
    const uint32_t cases = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 300u;
    std::mt19937 rng(20261020u);
    rt_denoise_params def;
    rt_denoise_default_params(&def);
    rt_variance_params vdef;
    CHECK(rt_variance_default_params(&vdef) == RT_OK && vdef.source == RT_VARIANCE_MOMENTS && vdef.radius >= 1 && vdef.radius <= 3, "defaults");
    CHECK(rt_variance_default_params(nullptr) == RT_ERR_INVALID_ARG, "null defaults");
    size_t pixels = 0;
    for (uint32_t t = 0; t < cases; ++t) {
        const uint32_t W = 1 + rng() % (t % 10 == 0 ? 90 : 24), rows = 1 + rng() % (t % 10 == 1 ? 70 : 20);
        const Strips s = RandomStrips(rng, W, rows);
        rt_denoise_params P = def;
        P.levels = 1 + rng() % 3;
        if (t % 3 == 1) P.k_normal = P.k_depth = P.k_albedo = P.k_coverage = 0.f;
        const rt_variance_params V{RT_VARIANCE_SPATIAL, 1u + t % 3u};
        const size_t npix = (size_t)W * rows;
        std::vector<float> rgb(npix * 3, NAN), var(npix, NAN), st(npix * 4, NAN);
        const int rc = rt_unit_denoise_variance_host(s.hdr.data(), nullptr, s.n, s.feat.data(), s.m, W, rows, &P, &V, rgb.data(), var.data(), st.data());
        CHECK(rc == RT_OK, "case %u: rc %d (%s)", t, rc, rtprep::LastError());
        std::vector<float> g(npix * 8);
        for (size_t i = 0; i < npix * 8; ++i) g[i] = s.feat[i] / (float)s.m;
        for (size_t p = 0; p < npix; ++p) {
            for (int c = 0; c < 3; ++c) {
                CHECK(st[4 * p + c] == s.hdr[3 * p + c] / (float)s.n, "case %u pixel %zu: c0", t, p);
                CHECK(std::isfinite(rgb[3 * p + c]), "case %u pixel %zu: colour not finite", t, p);
            }
            const float v0 = st[4 * p + 3];
            CHECK(std::isfinite(v0) && v0 >= 0.f && std::isfinite(var[p]) && var[p] >= 0.f, "case %u pixel %zu: v0 %g, den_var %g", t, p, v0, var[p]);
            double range2[3];
            const double want = SecondV0(s, st, g, P, (int)V.radius, (int)(p % W), (int)(p / W), range2);
            // binary32 sums of up to 49 terms of magnitude <= 16 and a difference of two such means: 1e-4 absolute covers the cancellation
            CHECK(std::fabs((double)v0 - want) <= 1e-4 + 1e-4 * want, "case %u pixel %zu: v0 %g, formed again %g", t, p, v0, want);
            CHECK((double)v0 <= range2[0] + range2[1] + range2[2] + 1e-4, "case %u pixel %zu: v0 %g beyond the window's range", t, p, v0);
        }
        pixels += npix;
        // the strip as rows [first_row, first_row + rows) of a taller image, through the temporal twin on an empty history
        {
            const uint32_t first_row = 1 + rng() % 7, H = first_row + rows + rng() % 5;
            rt_camera cam{};
            cam.origin[2] = 5.f;
            cam.x[0] = 1.f;
            cam.y[1] = 1.f;
            cam.origin_image_plane[2] = 4.f;
            cam.aperture = 0.f;
            cam.focal_length = 1.f;
            std::vector<float> rgb2(npix * 3, NAN), var2(npix, NAN), st2(npix * 4, NAN), g2(npix * 8, NAN);
            std::vector<uint32_t> len(npix, 7u), target(npix, 7u);
            const uint32_t fetch = t % 2 ? RT_TEMPORAL_FETCH_BILINEAR : RT_TEMPORAL_FETCH_NEAREST;
            const int rc2 = rt_unit_temporal_variance_host(s.hdr.data(), nullptr, s.n, s.feat.data(), s.m, s.ids.data(), W, H, first_row, rows, &cam, nullptr, nullptr,
                                                           nullptr, nullptr, nullptr, &P, nullptr, fetch, &V, rgb2.data(), var2.data(), st2.data(), g2.data(),
                                                           len.data(), target.data());
            CHECK(rc2 == RT_OK, "case %u: temporal twin rc %d (%s)", t, rc2, rtprep::LastError());
            CHECK(std::memcmp(st2.data(), st.data(), npix * 16) == 0, "case %u: band at row %u: prepared state differs", t, first_row);
            CHECK(std::memcmp(rgb2.data(), rgb.data(), npix * 12) == 0 && std::memcmp(var2.data(), var.data(), npix * 4) == 0, "case %u: band: den differs", t);
            CHECK(std::memcmp(g2.data(), g.data(), npix * 32) == 0, "case %u: band: guides differ", t);
            for (size_t p = 0; p < npix; ++p) CHECK(len[p] == 1u && target[p] == 0xffffffffu, "case %u pixel %zu: len %u target %u", t, p, len[p], target[p]);
        }
        // the moments source is rt_unit_denoise_host (n >= 2)
        if (s.n >= 2) {
            std::vector<float> sq(npix * 3);
            for (size_t i = 0; i < npix * 3; ++i) sq[i] = s.hdr[i] * s.hdr[i] / (float)s.n * 1.25f;
            const rt_variance_params M{RT_VARIANCE_MOMENTS, 99u};  // (the radius is not read)
            std::vector<float> r1(npix * 3, NAN), v1(npix, NAN), r2(npix * 3, NAN), v2(npix, NAN);
            CHECK(rt_unit_denoise_host(s.hdr.data(), sq.data(), s.n, s.feat.data(), s.m, W, rows, &P, r1.data(), v1.data()) == RT_OK, "case %u: moments", t);
            CHECK(rt_unit_denoise_variance_host(s.hdr.data(), sq.data(), s.n, s.feat.data(), s.m, W, rows, &P, t % 2 ? &M : nullptr, r2.data(), v2.data(), nullptr) ==
                      RT_OK,
                  "case %u: moments through the variance entry", t);
            CHECK(std::memcmp(r1.data(), r2.data(), npix * 12) == 0 && std::memcmp(v1.data(), v2.data(), npix * 4) == 0, "case %u: moments source differs", t);
        }
    }
    // a constant picture of power-of-two values: v0 == 0 exactly under any guides
    {
        const uint32_t W = 41, rows = 23;
        Strips s = RandomStrips(rng, W, rows);
        const size_t npix = (size_t)W * rows;
        for (size_t p = 0; p < npix; ++p) s.hdr[3 * p] = 0.5f * (float)s.n, s.hdr[3 * p + 1] = 2.f * (float)s.n, s.hdr[3 * p + 2] = 0.125f * (float)s.n;
        for (uint32_t R = 1; R <= 3; ++R) {
            const rt_variance_params V{RT_VARIANCE_SPATIAL, R};
            std::vector<float> rgb(npix * 3), var(npix), st(npix * 4);
            CHECK(rt_unit_denoise_variance_host(s.hdr.data(), nullptr, s.n, s.feat.data(), s.m, W, rows, &def, &V, rgb.data(), var.data(), st.data()) == RT_OK, "constant");
            for (size_t p = 0; p < npix; ++p) CHECK(st[4 * p + 3] == 0.f && var[p] == 0.f, "constant picture, R %u, pixel %zu: v0 %g", R, p, st[4 * p + 3]);
        }
    }
    // refusals
    {
        float z[8] = {0}, o3[3], o1[1], o4[4];
        rt_variance_params V{RT_VARIANCE_SPATIAL, 3};
        CHECK(rt_unit_denoise_variance_host(z, nullptr, 1, z, 1, 1, 1, nullptr, &V, o3, o1, o4) == RT_OK, "1 x 1, n = 1, null sq");
        CHECK(o4[3] == 0.f, "a lone pixel has no spread");
        CHECK(rt_unit_denoise_variance_host(z, nullptr, 0, z, 1, 1, 1, nullptr, &V, o3, o1, o4) == RT_ERR_SEQUENCE, "n == 0");
        CHECK(rt_unit_denoise_variance_host(z, nullptr, 1, z, 0, 1, 1, nullptr, &V, o3, o1, o4) == RT_ERR_SEQUENCE, "m == 0");
        CHECK(rt_unit_denoise_variance_host(nullptr, nullptr, 1, z, 1, 1, 1, nullptr, &V, o3, o1, o4) == RT_ERR_INVALID_ARG, "null hdr");
        for (uint32_t r : {0u, 4u, 0xffffffffu}) {
            V.radius = r;
            CHECK(rt_unit_denoise_variance_host(z, z, 2, z, 1, 1, 1, nullptr, &V, o3, o1, o4) == RT_ERR_INVALID_ARG, "radius %u", r);
        }
        V = rt_variance_params{2, 3};
        CHECK(rt_unit_denoise_variance_host(z, z, 2, z, 1, 1, 1, nullptr, &V, o3, o1, o4) == RT_ERR_INVALID_ARG, "unknown source");
        V = rt_variance_params{RT_VARIANCE_MOMENTS, 0};
        CHECK(rt_unit_denoise_variance_host(z, z, 2, z, 1, 1, 1, nullptr, &V, o3, o1, nullptr) == RT_OK, "moments: the radius is not read");
        CHECK(rt_unit_denoise_variance_host(z, nullptr, 2, z, 1, 1, 1, nullptr, &V, o3, o1, nullptr) == RT_ERR_INVALID_ARG, "moments: null sq");
        CHECK(rt_unit_denoise_variance_host(z, nullptr, 2, z, 1, 1, 1, nullptr, nullptr, o3, o1, nullptr) == RT_ERR_INVALID_ARG, "NULL vparams: null sq");
        CHECK(rt_unit_denoise_variance_host(z, z, 1, z, 1, 1, 1, nullptr, &V, o3, o1, nullptr) == RT_ERR_SEQUENCE, "moments: n == 1");
    }
    if (g_fail) {
        std::fprintf(stderr, "denoise_spatial_selftest: %d failures\n", g_fail);
        return 1;
    }
    std::printf("denoise_spatial_selftest ok: %u random cases, %zu pixels, radii 1..3\n", cases, pixels);
    return 0;
}
