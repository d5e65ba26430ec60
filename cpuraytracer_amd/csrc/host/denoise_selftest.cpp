// denoise_selftest.cpp -- the denoiser's host twin (rt_denoise_host.cpp over ../rt_denoise.h) in a program of its own: random strips
// and shapes with invariants no picture should break.  No HIP, no librt_hip.so; also built under ASan + UBSan (Makefile
// denoise_selftest_san), where every index the filter forms is checked.
//   - sw > 0 at every pixel of every level (the centre tap), so no output is a NaN that the inputs did not hold;
//   - finite in -> finite out, den_var >= 0;
//   - levels whose step exceeds the image (only the centre row / column of taps is left) still give every pixel;
//   - all k == 0, uniform picture: the picture is returned and the variance shrinks;
//   - the same strips cut into the parts of a random cyclic row set give the contiguous filter's bits (rt_unit_denoise_shards_host over
//     ../rt_rowset_map.h), whatever the padding rows hold;
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
#include "../rt_rowset_map.h"
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
    std::vector<float> hdr, sq, feat;
};

static Strips RandomStrips(std::mt19937& rng, uint32_t W, uint32_t rows) {
    Strips s;
    s.W = W;
    s.rows = rows;
    s.n = 2 + rng() % 15;
    s.m = 1 + rng() % 8;
    const size_t npix = (size_t)W * rows;
    s.hdr.resize(npix * 3);
    s.sq.resize(npix * 3);
    s.feat.resize(npix * 8);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    for (size_t p = 0; p < npix; ++p) {
        const uint32_t kind = rng() % 8;  // 0 black, 1 no variance, 2 Q < S^2 / n, else noisy
        for (int c = 0; c < 3; ++c) {
            float S = 0.f, Q = 0.f;
            for (uint32_t k = 0; k < s.n; ++k) {
                const float v = kind == 0 ? 0.f : (kind == 1 ? 0.5f : 4.f * u(rng) * u(rng));
                S += v;
                Q += v * v;
            }
            if (kind == 2) Q *= 0.5f;
            s.hdr[3 * p + c] = S;
            s.sq[3 * p + c] = Q;
        }
        const bool sky = rng() % 4 == 0;
        const float fm = (float)s.m;
        float* f = &s.feat[8 * p];
        for (int c = 0; c < 3; ++c) f[c] = u(rng) * fm;
        for (int c = 3; c < 6; ++c) f[c] = sky ? 0.f : (2.f * u(rng) - 1.f) * fm;
        f[6] = sky ? 0.f : 30.f * u(rng) * fm;
        f[7] = sky ? 0.f : (float)(1 + rng() % s.m);
    }
    return s;
}

int main(int argc, char** argv) {
    const uint32_t cases = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 300u;
    std::mt19937 rng(20261019u);
    rt_denoise_params def;
    CHECK(rt_denoise_default_params(&def) == RT_OK && def.levels == 3 && def.k_normal == 16.f && def.k_depth == 400.f && def.k_albedo == 64.f &&
              def.k_coverage == 16.f && def.k_colour == 1.f && def.var_floor == 1e-6f,
          "defaults");
    CHECK(rt_denoise_default_params(nullptr) == RT_ERR_INVALID_ARG, "null defaults");
    size_t pixels = 0;
    for (uint32_t t = 0; t < cases; ++t) {
        const uint32_t W = 1 + rng() % (t % 10 == 0 ? 90 : 24), rows = 1 + rng() % (t % 10 == 1 ? 70 : 20);
        const Strips s = RandomStrips(rng, W, rows);
        rt_denoise_params P = def;
        P.levels = 1 + rng() % 5;  // steps up to 16: beyond most of these shapes
        if (t % 3 == 1) P.k_normal = P.k_depth = P.k_albedo = P.k_coverage = P.k_colour = 0.f;
        if (t % 3 == 2) {
            std::uniform_real_distribution<float> u(0.f, 1.f);
            P.k_normal = 100.f * u(rng), P.k_depth = 1000.f * u(rng), P.k_albedo = 100.f * u(rng), P.k_coverage = 100.f * u(rng), P.k_colour = 10.f * u(rng);
            P.var_floor = 1e-8f + u(rng) * 1e-3f;
        }
        const size_t npix = (size_t)W * rows;
        std::vector<float> rgb(npix * 3, NAN), var(npix, NAN);
        const int rc = rt_unit_denoise_host(s.hdr.data(), s.sq.data(), s.n, s.feat.data(), s.m, W, rows, &P, rgb.data(), var.data());
        CHECK(rc == RT_OK, "case %u: rc %d (%s)", t, rc, rtprep::LastError());
        float lo = INFINITY, hi = -INFINITY;
        for (size_t p = 0; p < npix; ++p)
            for (int c = 0; c < 3; ++c) {
                const float m = s.hdr[3 * p + c] / (float)s.n;
                lo = m < lo ? m : lo;
                hi = m > hi ? m : hi;
            }
        for (size_t p = 0; p < npix; ++p) {
            for (int c = 0; c < 3; ++c) {
                const float v = rgb[3 * p + c];
                // sw > 0 or this is a NaN; a weighted mean with weights >= 0 stays inside the input's range up to rounding
                CHECK(std::isfinite(v), "case %u pixel %zu: colour not finite", t, p);
                CHECK(v >= lo - 1e-4f * (1.f + std::fabs(lo)) && v <= hi + 1e-4f * (1.f + std::fabs(hi)), "case %u pixel %zu: %g outside [%g, %g]", t, p, v, lo, hi);
            }
            CHECK(std::isfinite(var[p]) && var[p] >= 0.f, "case %u pixel %zu: variance %g", t, p, var[p]);
        }
        pixels += npix;
        // the same strips cut into the parts of a cyclic row set (rt_unit_denoise_shards_host): NaN in every padding row, and the buffers
        // end where the last owned row ends, so under ASan a read of the padding behind it is caught as well
        {
            rt_shard_parts sp{};
            sp.W = W;
            sp.rs = rt_rowset{(uint32_t)(rng() % 5), rows, (uint32_t)(1 + rng() % 5), 0, (uint32_t)(1 + rng() % 9)};
            sp.n = s.n;
            sp.m = s.m;
            const uint32_t most = rtd::rowset_max_shard_rows(rows, sp.rs.block_rows, sp.rs.nshards);
            sp.rows_max = most + rng() % 2;
            size_t used = 0;
            uint32_t sum = 0;
            for (uint32_t k = 0; k < sp.rs.nshards; ++k) {
                const uint32_t own = rtd::rowset_shard_rows(rows, sp.rs.block_rows, sp.rs.nshards, k);
                CHECK(own <= most, "case %u: shard %u owns %u rows, more than shard 0's %u", t, k, own, most);
                sum += own;
                if (own) used = ((size_t)k * sp.rows_max + own) * W;
            }
            CHECK(sum == rows, "case %u: the shards own %u of %u rows", t, sum, rows);
            std::vector<float> ph(used * 3, NAN), pq(used * 3, NAN), pf(used * 8, NAN);
            for (uint32_t y = 0; y < rows; ++y) {
                uint32_t k = 0, lr = 0;
                CHECK(rt_rowset_locate(sp.rs, y, &k, &lr) == RT_OK && k < sp.rs.nshards && lr < sp.rows_max, "case %u: row %u -> (%u, %u)", t, y, k, lr);
                const size_t dst = ((size_t)k * sp.rows_max + lr) * W, src = (size_t)y * W;
                CHECK(dst + W <= used, "case %u: row %u lies beyond the owned rows", t, y);
                for (size_t i = 0; i < (size_t)W * 3; ++i) ph[3 * dst + i] = s.hdr[3 * src + i], pq[3 * dst + i] = s.sq[3 * src + i];
                for (size_t i = 0; i < (size_t)W * 8; ++i) pf[8 * dst + i] = s.feat[8 * src + i];
            }
            std::vector<float> rgb2(npix * 3, NAN), var2(npix, NAN);
            const int rc2 = rt_unit_denoise_shards_host(ph.data(), pq.data(), pf.data(), &sp, &P, rgb2.data(), var2.data());
            CHECK(rc2 == RT_OK, "case %u: parts form rc %d (%s)", t, rc2, rtprep::LastError());
            CHECK(std::memcmp(rgb2.data(), rgb.data(), npix * 12) == 0 && std::memcmp(var2.data(), var.data(), npix * 4) == 0,
                  "case %u: %u x %u in %u shards of %u-row blocks differs from the contiguous filter", t, W, rows, sp.rs.nshards, sp.rs.block_rows);
        }
    }
    // the sums of one pixel, directly: sw >= the centre tap's 9/64 whatever the neighbours are
    {
        const rtd::DenoiseParams P{3, 16.f, 400.f, 64.f, 16.f, 1.f, 1e-6f};
        std::uniform_real_distribution<float> u(0.f, 1.f);
        for (int t = 0; t < 20000; ++t) {
            rtd::DenoiseState a{{u(rng), u(rng), u(rng)}, u(rng) * u(rng)}, b{{4.f * u(rng), u(rng), u(rng)}, u(rng)};
            float ga[8], gb[8];
            for (int k = 0; k < 8; ++k) ga[k] = u(rng), gb[k] = (t & 1) ? 0.f : u(rng);
            rtd::DenoiseSums S;
            rtd::denoise_begin(S);
            rtd::denoise_tap(P, 0.375f * 0.375f, a, ga, a, ga, S);
            CHECK(S.sw == 0.140625f, "centre tap weight %g", S.sw);
            rtd::denoise_tap(P, 0.25f * 0.0625f, a, ga, b, gb, S);
            CHECK(S.sw >= 0.140625f && S.sw <= 0.140625f + 0.015625f, "sw %g", S.sw);
        }
    }
    // all k == 0 on a uniform picture: the picture comes back, the variance of an interior pixel is (70/256)^2 v0 per level
    {
        const uint32_t W = 40, rows = 30, n = 4;
        const size_t npix = (size_t)W * rows;
        std::vector<float> hdr(npix * 3), sq(npix * 3), feat(npix * 8, 0.f), rgb(npix * 3), var(npix);
        for (size_t p = 0; p < npix; ++p)
            for (int c = 0; c < 3; ++c) hdr[3 * p + c] = 2.f, sq[3 * p + c] = 1.75f;  // samples {0, 0.5, 0.5, 1}: mean 0.5, variance 1/4 * 2/3
        rt_denoise_params P = def;
        P.levels = 1;
        P.k_normal = P.k_depth = P.k_albedo = P.k_coverage = P.k_colour = 0.f;
        CHECK(rt_unit_denoise_host(hdr.data(), sq.data(), n, feat.data(), 1, W, rows, &P, rgb.data(), var.data()) == RT_OK, "uniform");
        float est[2];
        rtd::noise_estimate(&hdr[0], &sq[0], n, 0.f, est);
        const double v0 = (double)est[0] * est[0], want = v0 * (70.0 / 256.0) * (70.0 / 256.0);
        const size_t mid = (size_t)15 * W + 20;
        CHECK(std::fabs(rgb[3 * mid] - 0.5f) < 1e-6f, "uniform colour %g", rgb[3 * mid]);
        CHECK(std::fabs(var[mid] - want) <= 64.0 * std::ldexp(1.0, -24) * want, "uniform variance %g, expected %g", var[mid], want);
        CHECK(var[0] > var[mid] && var[0] < v0, "a corner keeps fewer taps: %g vs %g", var[0], var[mid]);
    }
    // refusals
    {
        float z[8] = {0}, o3[3], o1[1];
        rt_denoise_params P = def;
        CHECK(rt_unit_denoise_host(z, z, 2, z, 1, 1, 1, nullptr, o3, o1) == RT_OK, "NULL params are the defaults");
        CHECK(rt_unit_denoise_host(nullptr, z, 2, z, 1, 1, 1, &P, o3, o1) == RT_ERR_INVALID_ARG, "null hdr");
        CHECK(rt_unit_denoise_host(z, z, 2, z, 1, 1, 1, &P, o3, nullptr) == RT_ERR_INVALID_ARG, "null out");
        CHECK(rt_unit_denoise_host(z, z, 2, z, 1, 0, 1, &P, o3, o1) == RT_ERR_INVALID_ARG, "W == 0");
        CHECK(rt_unit_denoise_host(z, z, 1, z, 1, 1, 1, &P, o3, o1) == RT_ERR_SEQUENCE, "n == 1");
        CHECK(rt_unit_denoise_host(z, z, 2, z, 0, 1, 1, &P, o3, o1) == RT_ERR_SEQUENCE, "m == 0");
        for (uint32_t lv : {0u, 6u}) {
            P = def;
            P.levels = lv;
            CHECK(rt_unit_denoise_host(z, z, 2, z, 1, 1, 1, &P, o3, o1) == RT_ERR_INVALID_ARG, "levels %u", lv);
        }
        for (float bad : {-1.f, NAN, INFINITY}) {
            float rt_denoise_params::*fields[] = {&rt_denoise_params::k_normal, &rt_denoise_params::k_depth,  &rt_denoise_params::k_albedo,
                                                   &rt_denoise_params::k_coverage, &rt_denoise_params::k_colour, &rt_denoise_params::var_floor};
            for (auto f : fields) {
                P = def;
                P.*f = bad;
                CHECK(rt_unit_denoise_host(z, z, 2, z, 1, 1, 1, &P, o3, o1) == RT_ERR_INVALID_ARG, "field value %g", bad);
            }
        }
        P = def;
        P.var_floor = 0.f;
        CHECK(rt_unit_denoise_host(z, z, 2, z, 1, 1, 1, &P, o3, o1) == RT_ERR_INVALID_ARG, "var_floor == 0");
    }
    if (g_fail) {
        std::fprintf(stderr, "denoise_selftest: %d failures\n", g_fail);
        return 1;
    }
    std::printf("denoise_selftest ok: %u random cases, %zu pixels, levels 1..5\n", cases, pixels);
    return 0;
}
