// rt_denoise_host.cpp -- the denoiser's arithmetic (../rt_denoise.h) compiled for the host: rt_unit_denoise_host, the twin the
// device is compared with bit for bit, its form over the gathered parts of a row-sharded picture (rt_unit_denoise_shards_host; the
// mapping is ../rt_rowset_map.h, which rt_rowset_locate exposes), and the parameter defaults.  Plain C++ with no HIP header, under the
// same floating-point contract as the kernels (-ffp-contract=off, IEEE division).  Needs no GPU.
#include <cstddef>
#include <string>
#include <vector>

#include "../../../include/rt_api.h"
#include "../rt_denoise.h"
#include "../rt_rowset_map.h"
#include "rt_denoise_host.h"
#include "rt_denoise_launch.h"
#include "rt_error.h"

using rtprep::Fail;

static_assert(sizeof(rt_denoise_params) == sizeof(rtd::DenoiseParams) && offsetof(rt_denoise_params, var_floor) == offsetof(rtd::DenoiseParams, var_floor),
              "rt_denoise_params is laid out like rtd::DenoiseParams");

// The levels over the prepared state a (b: the other buffer) and guides g of a W x rows picture; the last level's state goes out.
void rtdn::RunLevelsHost(std::vector<rtd::DenoiseState>& a, std::vector<rtd::DenoiseState>& b, const std::vector<float>& g, uint32_t W, uint32_t rows,
                         const rtd::DenoiseParams& P, float* out_rgb, float* out_var) {
    const size_t npix = (size_t)W * rows;
    const rtd::DenoiseState* in = a.data();
    rtd::DenoiseState* out = b.data();
    for (uint32_t l = 0; l < P.levels; ++l) {
        const int64_t step = (int64_t)1 << l;
        for (int64_t y = 0; y < (int64_t)rows; ++y) {
            for (int64_t x = 0; x < (int64_t)W; ++x) {
                const size_t p = (size_t)y * W + (size_t)x;
                rtd::DenoiseSums S;
                rtd::denoise_begin(S);
                for (int ta = 0; ta < 5; ++ta) {
                    const int64_t qy = y + (ta - 2) * step;
                    if (qy < 0 || qy >= (int64_t)rows) continue;
                    for (int tb = 0; tb < 5; ++tb) {
                        const int64_t qx = x + (tb - 2) * step;
                        if (qx < 0 || qx >= (int64_t)W) continue;
                        const size_t q = (size_t)qy * W + (size_t)qx;
                        rtd::denoise_tap(P, rtd::denoise_h(ta) * rtd::denoise_h(tb), in[p], &g[8 * p], in[q], &g[8 * q], S);
                    }
                }
                rtd::denoise_finish(S, out[p]);
            }
        }
        in = out;
        out = out == b.data() ? a.data() : b.data();
    }
    for (size_t p = 0; p < npix; ++p) {
        for (int k = 0; k < 3; ++k) out_rgb[3 * p + k] = in[p].c[k];
        out_var[p] = in[p].v;
    }
}

static_assert(sizeof(rt_variance_params) == sizeof(rtd::VarianceParams) && offsetof(rt_variance_params, radius) == offsetof(rtd::VarianceParams, radius),
              "rt_variance_params is laid out like rtd::VarianceParams");
static_assert(RT_VARIANCE_MOMENTS == rtd::kVarianceMoments && RT_VARIANCE_SPATIAL == rtd::kVarianceSpatial, "the sources of rt_api.h are those of rt_denoise.h");

namespace rtdn {

int CheckDenoiseParams(const char* who_, const rt_denoise_params* params, rtd::DenoiseParams* P) {
    rt_denoise_params def;
    rt_denoise_default_params(&def);
    if (!params) params = &def;
    *P = rtd::DenoiseParams{params->levels, params->k_normal, params->k_depth, params->k_albedo, params->k_coverage, params->k_colour, params->var_floor};
    if (!rtd::denoise_params_ok(*P))
        return Fail(RT_ERR_INVALID_ARG, std::string(who_) + ": levels must be 1..5, every k and var_floor finite and >= 0, var_floor > 0");
    return RT_OK;
}

// Where row y of the image's row range starts in the gathered parts (../rt_rowset_map.h).
size_t PartsRowStart(const ShardLayout& parts, uint32_t W, uint32_t y) {
    uint32_t shard, lr;
    rtd::rowset_locate(parts.blockRows, parts.nshards, y, shard, lr);
    return ((size_t)shard * parts.rowsMax + lr) * W;
}

int CheckVarianceParams(const char* who_, const rt_variance_params* vparams, rtd::VarianceParams* V) {
    *V = vparams ? rtd::VarianceParams{vparams->source, vparams->radius} : rtd::VarianceParams{rtd::kVarianceMoments, rtd::kVarianceMaxRadius};
    if (!rtd::variance_params_ok(*V))
        return Fail(RT_ERR_INVALID_ARG, std::string(who_) + ": source must be RT_VARIANCE_MOMENTS (0) or RT_VARIANCE_SPATIAL (1), and under it radius 1..3");
    return RT_OK;
}

// The spatial prepare pass as rt_denoise_prepare_spatial_kernel runs it: c0 and g of every pixel first, then the window's taps.  parts:
// hdr and feat8 are gathered parts and a row of the range is read where the mapping puts it (rt_denoise_prepare_spatial_shards_kernel);
// a and g are in image order either way, so the taps do not see the difference.
void PrepareSpatialHost(const float* hdr, uint32_t n, const float* feat8, uint32_t m, uint32_t W, uint32_t rows, const ShardLayout* parts,
                        const rtd::DenoiseParams& P, uint32_t radius, std::vector<rtd::DenoiseState>& a, std::vector<float>& g) {
    for (uint32_t y = 0; y < rows; ++y) {
        const size_t src = parts ? PartsRowStart(*parts, W, y) : (size_t)y * W, dst = (size_t)y * W;
        for (size_t x = 0; x < W; ++x) {
            rtd::denoise_prepare_mean(hdr + 3 * (src + x), n, feat8 + 8 * (src + x), m, a[dst + x].c, &g[8 * (dst + x)]);
            a[dst + x].v = 0.0f;
        }
    }
    const int64_t R = (int64_t)radius;
    for (int64_t y = 0; y < (int64_t)rows; ++y) {
        for (int64_t x = 0; x < (int64_t)W; ++x) {
            const size_t p = (size_t)y * W + (size_t)x;
            rtd::SpatialSums S;
            rtd::spatial_begin(S);
            for (int64_t ta = 0; ta <= 2 * R; ++ta) {
                const int64_t qy = y + ta - R;
                if (qy < 0 || qy >= (int64_t)rows) continue;
                for (int64_t tb = 0; tb <= 2 * R; ++tb) {
                    const int64_t qx = x + tb - R;
                    if (qx < 0 || qx >= (int64_t)W) continue;
                    const size_t q = (size_t)qy * W + (size_t)qx;
                    rtd::spatial_tap(P, &g[8 * p], a[q].c, &g[8 * q], S);
                }
            }
            a[p].v = rtd::spatial_finish(S);
        }
    }
}

// (CheckShardFrame, the same for an rt_shard_frame, ends with this one and lives in rt_temporal_host.cpp, beside the temporal parameters'
// checks it calls: denoise_selftest links this file without that one)
// (spatial: the spatial variance source -- sq is not looked at, and one sample is enough)
int CheckShardParts(const char* who_, const rt_shard_parts* parts, const rt_denoise_params* params, bool devicePointers, rtd::DenoiseParams* P, bool spatial) {
    const std::string who(who_);
    if (!parts || !P) return Fail(RT_ERR_INVALID_ARG, who + ": null argument");
    if (devicePointers && (!parts->hdr || (!parts->sq && !spatial) || !parts->feat)) return Fail(RT_ERR_INVALID_ARG, who + ": null parts");
    const rt_rowset rs = parts->rs;
    if (parts->W == 0 || rs.num_rows == 0 || rs.nshards == 0 || rs.block_rows == 0)
        return Fail(RT_ERR_INVALID_ARG, who + ": W, rs.num_rows, rs.nshards and rs.block_rows must not be 0");
    if ((uint64_t)parts->W * rs.num_rows > (1ull << 31)) return Fail(RT_ERR_INVALID_ARG, who + ": more than 2^31 pixels");
    if ((rs.num_rows + kTileH - 1u) / kTileH > 65535u) return Fail(RT_ERR_INVALID_ARG, who + ": more than 524,280 rows");
    if (parts->rows_max < rtd::rowset_max_shard_rows(rs.num_rows, rs.block_rows, rs.nshards))
        return Fail(RT_ERR_INVALID_ARG, who + ": rows_max is below the rows of the largest shard");
    if (devicePointers && (reinterpret_cast<uintptr_t>(parts->feat) & 15u) != 0) return Fail(RT_ERR_INVALID_ARG, who + ": feat is not 16-byte aligned");
    if (const int rc = CheckDenoiseParams(who_, params, P)) return rc;
    if (spatial ? parts->n == 0 : parts->n < 2)
        return Fail(RT_ERR_SEQUENCE, who + (spatial ? ": the parts hold no sample" : ": the noise estimate needs at least 2 samples per pixel"));
    if (parts->m == 0) return Fail(RT_ERR_SEQUENCE, who + ": the feature parts hold no sample");
    return RT_OK;
}

}  // namespace rtdn

extern "C" {

int rt_denoise_default_params(rt_denoise_params* out) {
    if (!out) return Fail(RT_ERR_INVALID_ARG, "rt_denoise_default_params: null argument");
    out->levels = 3;
    out->k_normal = 16.0f;
    out->k_depth = 400.0f;
    out->k_albedo = 64.0f;
    out->k_coverage = 16.0f;
    out->k_colour = 1.0f;
    out->var_floor = 1e-6f;
    return RT_OK;
}

// The twin of either entry (who: its name for the messages; vparams == NULL: the moments source).
static int DenoiseHost(const char* who_, const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, uint32_t W, uint32_t rows,
                       const rt_denoise_params* params, const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4) {
    const std::string who(who_);
    rtd::VarianceParams V{};
    int rc = rtdn::CheckVarianceParams(who_, vparams, &V);
    if (rc != RT_OK) return rc;
    const bool spatial = V.source == rtd::kVarianceSpatial;
    if (!hdr || (!sq && !spatial) || !feat8 || !out_rgb || !out_var) return Fail(RT_ERR_INVALID_ARG, who + ": null buffer");
    if (W == 0 || rows == 0 || (uint64_t)W * rows > (1ull << 31)) return Fail(RT_ERR_INVALID_ARG, who + ": empty or too large strip");
    rtd::DenoiseParams P{};
    if ((rc = rtdn::CheckDenoiseParams(who_, params, &P)) != RT_OK) return rc;
    if (spatial ? n == 0 : n < 2) return Fail(RT_ERR_SEQUENCE, who + (spatial ? ": the strips hold no sample" : ": the noise estimate needs at least 2 samples per pixel"));
    if (m == 0) return Fail(RT_ERR_SEQUENCE, who + ": the feature strips hold no sample");
    const size_t npix = (size_t)W * rows;
    std::vector<rtd::DenoiseState> a(npix), b(npix);
    std::vector<float> g(npix * 8);
    if (spatial)
        rtdn::PrepareSpatialHost(hdr, n, feat8, m, W, rows, nullptr, P, V.radius, a, g);
    else
        for (size_t p = 0; p < npix; ++p) rtd::denoise_prepare(hdr + 3 * p, sq + 3 * p, n, feat8 + 8 * p, m, a[p], &g[8 * p]);
    if (out_state4)
        for (size_t p = 0; p < npix; ++p) {
            for (int k = 0; k < 3; ++k) out_state4[4 * p + k] = a[p].c[k];
            out_state4[4 * p + 3] = a[p].v;
        }
    rtdn::RunLevelsHost(a, b, g, W, rows, P, out_rgb, out_var);
    return RT_OK;
}

int rt_unit_denoise_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, uint32_t W, uint32_t rows,
                         const rt_denoise_params* params, float* out_rgb, float* out_var) {
    return DenoiseHost("rt_unit_denoise_host", hdr, sq, n, feat8, m, W, rows, params, nullptr, out_rgb, out_var, nullptr);
}

// rt_unit_denoise_host with the variance source chosen.
int rt_unit_denoise_variance_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, uint32_t W, uint32_t rows,
                                  const rt_denoise_params* params, const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4) {
    return DenoiseHost("rt_unit_denoise_variance_host", hdr, sq, n, feat8, m, W, rows, params, vparams, out_rgb, out_var, out_state4);
}

int rt_variance_default_params(rt_variance_params* out) {
    if (!out) return Fail(RT_ERR_INVALID_ARG, "rt_variance_default_params: null argument");
    out->source = RT_VARIANCE_MOMENTS;
    out->radius = 1;  // (docs/EXPERIMENTS.md, the spatial-variance grid: the 3 x 3 window beat the wider ones on both measures, and costs least)
    return RT_OK;
}

int rt_rowset_locate(rt_rowset rs, uint32_t image_row, uint32_t* shard, uint32_t* local_row) {
    if (!shard || !local_row) return Fail(RT_ERR_INVALID_ARG, "rt_rowset_locate: null argument");
    if (rs.block_rows == 0 || rs.nshards == 0) return Fail(RT_ERR_INVALID_ARG, "rt_rowset_locate: block_rows and nshards must not be 0");
    if (image_row >= rs.num_rows) return Fail(RT_ERR_INVALID_ARG, "rt_rowset_locate: the row lies beyond the row range");
    rtd::rowset_locate(rs.block_rows, rs.nshards, image_row, *shard, *local_row);
    return RT_OK;
}

// The prepare pass reads every pixel through the mapping, as rt_denoise_prepare_shards_kernel (spatial source:
// rt_denoise_prepare_spatial_shards_kernel) does; the levels are the same code.  (vparams == NULL: the moments source.)
static int DenoiseShardsHost(const char* who_, const float* hdr, const float* sq, const float* feat8, const rt_shard_parts* shape, const rt_denoise_params* params,
                             const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4) {
    rtd::VarianceParams V{};
    int rc = rtdn::CheckVarianceParams(who_, vparams, &V);
    if (rc != RT_OK) return rc;
    const bool spatial = V.source == rtd::kVarianceSpatial;
    if (!hdr || (!sq && !spatial) || !feat8 || !out_rgb || !out_var) return Fail(RT_ERR_INVALID_ARG, std::string(who_) + ": null buffer");
    rtd::DenoiseParams P{};
    if ((rc = rtdn::CheckShardParts(who_, shape, params, false, &P, spatial)) != RT_OK) return rc;
    const uint32_t W = shape->W, rows = shape->rs.num_rows;
    const size_t npix = (size_t)W * rows;
    std::vector<rtd::DenoiseState> a(npix), b(npix);
    std::vector<float> g(npix * 8);
    const rtdn::ShardLayout layout{shape->rows_max, shape->rs.block_rows, shape->rs.nshards};
    if (spatial)
        rtdn::PrepareSpatialHost(hdr, shape->n, feat8, shape->m, W, rows, &layout, P, V.radius, a, g);
    else
        for (uint32_t y = 0; y < rows; ++y) {
            const size_t src = rtdn::PartsRowStart(layout, W, y), dst = (size_t)y * W;
            for (size_t x = 0; x < W; ++x)
                rtd::denoise_prepare(hdr + 3 * (src + x), sq + 3 * (src + x), shape->n, feat8 + 8 * (src + x), shape->m, a[dst + x], &g[8 * (dst + x)]);
        }
    if (out_state4)
        for (size_t p = 0; p < npix; ++p) {
            for (int k = 0; k < 3; ++k) out_state4[4 * p + k] = a[p].c[k];
            out_state4[4 * p + 3] = a[p].v;
        }
    rtdn::RunLevelsHost(a, b, g, W, rows, P, out_rgb, out_var);
    return RT_OK;
}

int rt_unit_denoise_shards_host(const float* hdr, const float* sq, const float* feat8, const rt_shard_parts* shape, const rt_denoise_params* params,
                                float* out_rgb, float* out_var) {
    return DenoiseShardsHost("rt_unit_denoise_shards_host", hdr, sq, feat8, shape, params, nullptr, out_rgb, out_var, nullptr);
}

// rt_unit_denoise_shards_host with the variance source chosen (the twin of rt_denoise_shards_variance); sq may be NULL under the spatial one.
int rt_unit_denoise_shards_variance_host(const float* hdr, const float* sq, const float* feat8, const rt_shard_parts* shape, const rt_denoise_params* params,
                                         const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4) {
    return DenoiseShardsHost("rt_unit_denoise_shards_variance_host", hdr, sq, feat8, shape, params, vparams, out_rgb, out_var, out_state4);
}

}  // extern "C"
