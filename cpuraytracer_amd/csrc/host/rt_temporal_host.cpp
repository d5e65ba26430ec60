// rt_temporal_host.cpp -- temporal accumulation (../rt_temporal.h) compiled for the host: rt_unit_temporal_host and
// rt_unit_temporal_host_fetch, the twins the device is compared with bit for bit -- one frame step (prepare, reproject, gather with
// the nearest or the bilinear fetch, validate, blend) plus the levels of rt_unit_denoise_host's filter (rtdn::RunLevelsHost,
// rt_denoise_host.cpp) --, their form over the gathered parts of a row-sharded picture (rt_unit_temporal_shards_host, the twin of
// rt_denoise_shards_temporal; the mapping is ../rt_rowset_map.h), what that entry and its twin refuse (rtdn::CheckShardFrame) and the
// parameter defaults of either fetch.  Plain C++ with no HIP header, under the same floating-point
// contract as the kernels (-ffp-contract=off, IEEE division).  Needs no GPU.
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "../../../include/rt_api.h"
#include "../rt_rowset_map.h"
#include "../rt_temporal.h"
#include "rt_denoise_host.h"
#include "rt_denoise_launch.h"
#include "rt_error.h"

using rtprep::Fail;

static_assert(sizeof(rt_temporal_params) == sizeof(rtd::TemporalParams) && offsetof(rt_temporal_params, coverage_tol) == offsetof(rtd::TemporalParams, coverage_tol),
              "rt_temporal_params is laid out like rtd::TemporalParams");

namespace rtdn {

int CheckTemporalParams(const char* who_, const rt_temporal_params* tparams, rtd::TemporalParams* T) {
    rt_temporal_params def;
    rt_temporal_default_params(&def);
    if (!tparams) tparams = &def;
    *T = rtd::TemporalParams{tparams->max_history, tparams->use_id, tparams->depth_tol, tparams->normal_tol, tparams->coverage_tol};
    if (!rtd::temporal_params_ok(*T))
        return Fail(RT_ERR_INVALID_ARG, std::string(who_) + ": max_history must be 1..64, every tolerance finite and >= 0");
    return RT_OK;
}

int CheckTemporalParamsFetch(const char* who_, const rt_temporal_params* tparams, uint32_t fetch, rtd::TemporalParams* T) {
    if (!rtd::temporal_fetch_ok(fetch))
        return Fail(RT_ERR_INVALID_ARG, std::string(who_) + ": fetch must be RT_TEMPORAL_FETCH_NEAREST (1) or RT_TEMPORAL_FETCH_BILINEAR (4)");
    rt_temporal_params def;
    rt_temporal_default_params_fetch(fetch, &def);
    return CheckTemporalParams(who_, tparams ? tparams : &def, T);
}

rtd::TemporalCam CamOf(const rt_camera& c) {
    rtd::TemporalCam C;
    rtd::temporal_cam(c.origin, c.x, c.y, c.origin_image_plane, C);
    return C;
}

// Beside CheckShardParts (rt_denoise_host.cpp), which it ends with: the frame's own fields first, so that every RT_ERR_INVALID_ARG
// comes before the sample counts' RT_ERR_SEQUENCE.
int CheckShardFrame(const char* who_, const rt_shard_frame* frame, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                    bool devicePointers, rtd::DenoiseParams* P, rtd::TemporalParams* T, rtd::TemporalGeom* G, bool spatial) {
    const std::string who(who_);
    if (!frame || !P || !T || !G) return Fail(RT_ERR_INVALID_ARG, who + ": null argument");
    if (devicePointers && !frame->ids) return Fail(RT_ERR_INVALID_ARG, who + ": null ids");
    if (devicePointers && (reinterpret_cast<uintptr_t>(frame->ids) & 3u) != 0) return Fail(RT_ERR_INVALID_ARG, who + ": ids is not 4-byte aligned");
    int rc = CheckTemporalParamsFetch(who_, tparams, fetch, T);
    if (rc != RT_OK) return rc;
    const rt_rowset& rs = frame->parts.rs;
    if (rs.num_rows != 0 && frame->parts.W != 0) {  // (an empty picture is CheckShardParts' to name)
        *G = rtd::TemporalGeom{frame->parts.W, frame->H, rs.first_row, rs.num_rows};
        if (!rtd::temporal_geom_ok(*G)) return Fail(RT_ERR_INVALID_ARG, who + ": W or H above 2^24, or H == 0");
        if ((uint64_t)rs.first_row + rs.num_rows > frame->H) return Fail(RT_ERR_INVALID_ARG, who + ": rows beyond the image (H < rs.first_row + rs.num_rows)");
    }
    const rt_camera& c = frame->camera;
    bool finite = std::isfinite(c.aperture) && std::isfinite(c.focal_length);
    for (int k = 0; k < 3; ++k)
        finite = finite && std::isfinite(c.origin[k]) && std::isfinite(c.x[k]) && std::isfinite(c.y[k]) && std::isfinite(c.origin_image_plane[k]);
    if (!finite) return Fail(RT_ERR_INVALID_ARG, who + ": a field of the camera is not finite");
    return CheckShardParts(who_, &frame->parts, params, devicePointers, P, spatial);
}

}  // namespace rtdn

extern "C" {

int rt_temporal_default_params(rt_temporal_params* out) {
    if (!out) return Fail(RT_ERR_INVALID_ARG, "rt_temporal_default_params: null argument");
    out->max_history = 2;  // (nearest-pixel fetches drift, a longer history loses more than it averages away)
    out->use_id = 1;
    out->depth_tol = 0.1f;
    out->normal_tol = 0.1f;
    out->coverage_tol = 0.25f;
    return RT_OK;
}

int rt_temporal_default_params_fetch(uint32_t fetch, rt_temporal_params* out) {
    if (!out) return Fail(RT_ERR_INVALID_ARG, "rt_temporal_default_params_fetch: null argument");
    if (!rtd::temporal_fetch_ok(fetch))
        return Fail(RT_ERR_INVALID_ARG, "rt_temporal_default_params_fetch: fetch must be RT_TEMPORAL_FETCH_NEAREST (1) or RT_TEMPORAL_FETCH_BILINEAR (4)");
    rt_temporal_default_params(out);
    // (docs/EXPERIMENTS.md, the fetch x max_history grid: interpolated taps drift less, so one more frame of history still pays)
    if (fetch == RT_TEMPORAL_FETCH_BILINEAR) out->max_history = 3;
    return RT_OK;
}

}  // extern "C"

// The frame step over every pixel plus the levels, for either fetch, after the entry's checks.  parts == NULL: hdr, sq, feat8 and ids
// are the strip in image order; else they are the gathered parts, and pixel (x, ly) of the row range is read where the mapping
// (../rt_rowset_map.h) puts its row, as rt_denoise_prepare_shards_temporal_kernel reads it.  The history and every output are in image
// order either way.
static void TemporalRun(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, const rtd::TemporalGeom& G,
                        const rtdn::ShardLayout* parts, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4, const float* hist_guides8,
                        const uint32_t* hist_ids, const uint32_t* hist_len, const rtd::DenoiseParams& P, const rtd::TemporalParams& T, uint32_t fetch,
                        float* out_rgb, float* out_var, float* out_state4, float* out_guides8, uint32_t* out_len, uint32_t* out_target,
                        const rtd::VarianceParams V = rtd::VarianceParams{rtd::kVarianceMoments, 0}) {
    const uint32_t W = G.W, first_row = G.first_row, num_rows = G.num_rows;
    const size_t npix = (size_t)W * num_rows;
    const rtd::TemporalCam C = rtdn::CamOf(*camera);
    const rtd::TemporalCam Cp = hist_len ? rtdn::CamOf(*hist_camera) : C;
    std::vector<rtd::DenoiseState> a(npix), b(npix);
    std::vector<float> g(npix * 8);
    // (the spatial source: the whole picture's (c0, v0) and g first, in image order, as the device's extra pass leaves them)
    const bool spatial = V.source == rtd::kVarianceSpatial;
    if (spatial) rtdn::PrepareSpatialHost(hdr, n, feat8, m, W, num_rows, parts, P, V.radius, a, g);
    for (uint32_t ly = 0; ly < num_rows; ++ly) {
        const size_t row = parts ? rtdn::PartsRowStart(*parts, W, ly) : (size_t)ly * W;  // where the row's current-frame pixels start
        for (uint32_t x = 0; x < W; ++x) {
            const size_t p = (size_t)ly * W + x, src = row + x;
            rtd::DenoiseState s;
            float* gp = &g[8 * p];
            if (spatial)
                s = a[p];
            else
                rtd::denoise_prepare(hdr + 3 * src, sq + 3 * src, n, feat8 + 8 * src, m, s, gp);
            const uint32_t id = ids[src];
            uint32_t len = 1u, target = rtd::kTemporalNoTarget;
            uint32_t xi = 0, yi = 0;
            float dist = 0.f;
            float fx = 0.f, fy = 0.f;
            if (hist_len && fetch == RT_TEMPORAL_FETCH_BILINEAR) {
                if (rtd::temporal_reproject_point(G, C, Cp, x, first_row + ly, gp, fx, fy, xi, yi, dist)) {
                    rtd::TemporalTaps B;
                    rtd::temporal_taps(fx, fy, xi, yi, B);
                    rtd::TemporalGather S;
                    rtd::temporal_gather_begin(S);
                    for (int k = 0; k < 4; ++k) {
                        uint32_t q = 0;
                        const float w = rtd::temporal_tap_weight(B, k);
                        if (!(rtd::temporal_tap_index(G, B, k, q) && w > 0.f)) continue;
                        if (!rtd::temporal_validate(T, gp, id, dist, hist_guides8 + 8 * (size_t)q, hist_ids[q], hist_len[q])) continue;
                        rtd::DenoiseState st;
                        for (int c = 0; c < 3; ++c) st.c[c] = hist_state4[4 * (size_t)q + c];
                        st.v = hist_state4[4 * (size_t)q + 3];
                        rtd::temporal_gather_tap(S, w, st, hist_len[q], q);
                    }
                    rtd::DenoiseState sh{};
                    uint32_t lh = 0u;
                    const bool ok = rtd::temporal_gather_finish(S, sh, lh);
                    len = rtd::temporal_blend(T, ok, s, sh, lh);
                    if (ok) target = S.target;
                }
            } else if (hist_len && rtd::temporal_reproject(G, C, Cp, x, first_row + ly, gp, xi, yi, dist)) {
                const size_t q = (size_t)(yi - first_row) * W + xi;
                rtd::DenoiseState sh;
                for (int k = 0; k < 3; ++k) sh.c[k] = hist_state4[4 * q + k];
                sh.v = hist_state4[4 * q + 3];
                const bool ok = rtd::temporal_validate(T, gp, id, dist, hist_guides8 + 8 * q, hist_ids[q], hist_len[q]);
                len = rtd::temporal_blend(T, ok, s, sh, hist_len[q]);
                if (ok) target = (uint32_t)q;
            }
            a[p] = s;
            if (out_state4) {
                for (int k = 0; k < 3; ++k) out_state4[4 * p + k] = s.c[k];
                out_state4[4 * p + 3] = s.v;
            }
            if (out_len) out_len[p] = len;
            if (out_target) out_target[p] = target;
        }
    }
    if (out_guides8)
        for (size_t i = 0; i < npix * 8; ++i) out_guides8[i] = g[i];
    if (out_rgb || out_var) {
        std::vector<float> rgb(npix * 3), var(npix);
        rtdn::RunLevelsHost(a, b, g, W, num_rows, P, rgb.data(), var.data());
        if (out_rgb)
            for (size_t i = 0; i < npix * 3; ++i) out_rgb[i] = rgb[i];
        if (out_var)
            for (size_t i = 0; i < npix; ++i) out_var[i] = var[i];
    }
}

// One frame step plus the levels, for either fetch (who: the entry's name for the messages).
static int TemporalHost(const char* who, const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, uint32_t W,
                        uint32_t H, uint32_t first_row, uint32_t num_rows, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4,
                        const float* hist_guides8, const uint32_t* hist_ids, const uint32_t* hist_len, const rt_denoise_params* params,
                        const rt_temporal_params* tparams, uint32_t fetch, float* out_rgb, float* out_var, float* out_state4, float* out_guides8,
                        uint32_t* out_len, uint32_t* out_target, const rt_variance_params* vparams = nullptr) {
    rtd::VarianceParams V{};
    if (const int rcv = rtdn::CheckVarianceParams(who, vparams, &V)) return rcv;
    const bool spatial = V.source == rtd::kVarianceSpatial;
    if (!hdr || (!sq && !spatial) || !feat8 || !ids || !camera) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    if (hist_len && (!hist_camera || !hist_state4 || !hist_guides8 || !hist_ids))
        return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": a history (hist_len != NULL) needs its camera, state, guides and ids");
    const rtd::TemporalGeom G{W, H, first_row, num_rows};
    if (!rtd::temporal_geom_ok(G) || (uint64_t)first_row + num_rows > H || (uint64_t)W * num_rows > (1ull << 31))
        return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": empty or too large strip, or rows beyond the image");
    rtd::DenoiseParams P{};
    rtd::TemporalParams T{};
    int rc = rtdn::CheckDenoiseParams(who, params, &P);
    if (rc != RT_OK || (rc = rtdn::CheckTemporalParamsFetch(who, tparams, fetch, &T)) != RT_OK) return rc;
    if (spatial && n == 0) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": the strips hold no sample");
    if (!spatial && n < 2) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": the noise estimate needs at least 2 samples per pixel");
    if (m == 0) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": the feature strips hold no sample");
    TemporalRun(hdr, sq, n, feat8, m, ids, G, nullptr, camera, hist_camera, hist_state4, hist_guides8, hist_ids, hist_len, P, T, fetch, out_rgb, out_var,
                out_state4, out_guides8, out_len, out_target, V);
    return RT_OK;
}

extern "C" {

int rt_unit_temporal_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, uint32_t W, uint32_t H,
                          uint32_t first_row, uint32_t num_rows, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4,
                          const float* hist_guides8, const uint32_t* hist_ids, const uint32_t* hist_len, const rt_denoise_params* params,
                          const rt_temporal_params* tparams, float* out_rgb, float* out_var, float* out_state4, float* out_guides8, uint32_t* out_len,
                          uint32_t* out_target) {
    return TemporalHost("rt_unit_temporal_host", hdr, sq, n, feat8, m, ids, W, H, first_row, num_rows, camera, hist_camera, hist_state4, hist_guides8, hist_ids,
                        hist_len, params, tparams, RT_TEMPORAL_FETCH_NEAREST, out_rgb, out_var, out_state4, out_guides8, out_len, out_target);
}

int rt_unit_temporal_host_fetch(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, uint32_t W, uint32_t H,
                                uint32_t first_row, uint32_t num_rows, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4,
                                const float* hist_guides8, const uint32_t* hist_ids, const uint32_t* hist_len, const rt_denoise_params* params,
                                const rt_temporal_params* tparams, uint32_t fetch, float* out_rgb, float* out_var, float* out_state4, float* out_guides8,
                                uint32_t* out_len, uint32_t* out_target) {
    return TemporalHost("rt_unit_temporal_host_fetch", hdr, sq, n, feat8, m, ids, W, H, first_row, num_rows, camera, hist_camera, hist_state4, hist_guides8,
                        hist_ids, hist_len, params, tparams, fetch, out_rgb, out_var, out_state4, out_guides8, out_len, out_target);
}

// rt_unit_temporal_host_fetch with the variance source chosen (the twin of rt_denoise_temporal_variance); sq may be NULL under the spatial one.
int rt_unit_temporal_variance_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, uint32_t W, uint32_t H,
                                   uint32_t first_row, uint32_t num_rows, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4,
                                   const float* hist_guides8, const uint32_t* hist_ids, const uint32_t* hist_len, const rt_denoise_params* params,
                                   const rt_temporal_params* tparams, uint32_t fetch, const rt_variance_params* vparams, float* out_rgb, float* out_var,
                                   float* out_state4, float* out_guides8, uint32_t* out_len, uint32_t* out_target) {
    return TemporalHost("rt_unit_temporal_variance_host", hdr, sq, n, feat8, m, ids, W, H, first_row, num_rows, camera, hist_camera, hist_state4, hist_guides8,
                        hist_ids, hist_len, params, tparams, fetch, out_rgb, out_var, out_state4, out_guides8, out_len, out_target, vparams);
}

}  // extern "C"

// The sharded form: the same step, the current frame read through the mapping (TemporalRun).  (vparams == NULL: the moments source.)
static int TemporalShardsHost(const char* who, const float* hdr, const float* sq, const float* feat8, const uint32_t* ids, const rt_shard_frame* shape,
                              const rt_camera* hist_camera, const float* hist_state4, const float* hist_guides8, const uint32_t* hist_ids,
                              const uint32_t* hist_len, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                              const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4, float* out_guides8, uint32_t* out_len,
                              uint32_t* out_target) {
    rtd::VarianceParams V{};
    if (const int rcv = rtdn::CheckVarianceParams(who, vparams, &V)) return rcv;
    const bool spatial = V.source == rtd::kVarianceSpatial;
    if (!hdr || (!sq && !spatial) || !feat8 || !ids) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    if (hist_len && (!hist_camera || !hist_state4 || !hist_guides8 || !hist_ids))
        return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": a history (hist_len != NULL) needs its camera, state, guides and ids");
    rtd::DenoiseParams P{};
    rtd::TemporalParams T{};
    rtd::TemporalGeom G{};
    const int rc = rtdn::CheckShardFrame(who, shape, params, tparams, fetch, false, &P, &T, &G, spatial);
    if (rc != RT_OK) return rc;
    const rtdn::ShardLayout layout{shape->parts.rows_max, shape->parts.rs.block_rows, shape->parts.rs.nshards};
    TemporalRun(hdr, sq, shape->parts.n, feat8, shape->parts.m, ids, G, &layout, &shape->camera, hist_camera, hist_state4, hist_guides8, hist_ids, hist_len, P,
                T, fetch, out_rgb, out_var, out_state4, out_guides8, out_len, out_target, V);
    return RT_OK;
}

extern "C" {

int rt_unit_temporal_shards_host(const float* hdr, const float* sq, const float* feat8, const uint32_t* ids, const rt_shard_frame* shape,
                                 const rt_camera* hist_camera, const float* hist_state4, const float* hist_guides8, const uint32_t* hist_ids,
                                 const uint32_t* hist_len, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                                 float* out_rgb, float* out_var, float* out_state4, float* out_guides8, uint32_t* out_len, uint32_t* out_target) {
    return TemporalShardsHost("rt_unit_temporal_shards_host", hdr, sq, feat8, ids, shape, hist_camera, hist_state4, hist_guides8, hist_ids, hist_len, params,
                              tparams, fetch, nullptr, out_rgb, out_var, out_state4, out_guides8, out_len, out_target);
}

// rt_unit_temporal_shards_host with the variance source chosen (the twin of rt_denoise_shards_temporal_variance); sq may be NULL under the
// spatial one.
int rt_unit_temporal_shards_variance_host(const float* hdr, const float* sq, const float* feat8, const uint32_t* ids, const rt_shard_frame* shape,
                                          const rt_camera* hist_camera, const float* hist_state4, const float* hist_guides8, const uint32_t* hist_ids,
                                          const uint32_t* hist_len, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                                          const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4, float* out_guides8,
                                          uint32_t* out_len, uint32_t* out_target) {
    return TemporalShardsHost("rt_unit_temporal_shards_variance_host", hdr, sq, feat8, ids, shape, hist_camera, hist_state4, hist_guides8, hist_ids, hist_len,
                              params, tparams, fetch, vparams, out_rgb, out_var, out_state4, out_guides8, out_len, out_target);
}

}  // extern "C"
