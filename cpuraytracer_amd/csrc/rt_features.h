// rt_features.h -- first-hit feature buffers (DESIGN.md "Feature buffers"): what one sample of a pixel adds to the strip.
//
// The sample's ray is the path's primary ray and its hit the contract's closest hit (rt_kernels.h rt_features_kernel composes
// gen_primary_ray and the production scans).  From the hit record and the hit sphere's material this file derives the sample's
// feature vector v[8] = albedo rgb, normal xyz, depth, coverage and its object id:
//     hit, OPAQUE / METAL / EMISSIVE   Texture::Evaluate(uv) of the material's texture | normal | t | 1 | original sphere index
//     hit, TRANSPARENT                 (1, 1, 1)                                       | normal | t | 1 | original sphere index
//     miss                             the sky texture at uv (0, 0)                    | 0 0 0  | 0 | 0 | 0xffffffff
// The strip keeps feat[c] = feat[c] + v[c] in binary32, added in increasing s, and the id of the sample added last.
//
// No arithmetic happens here beyond eval_texture's (rt_texture.h).  The file is compiled with -ffp-contract=off for the device
// and for the host (rt_unit_features_host), so the kernel and the host twin give the same bits.
#pragma once

#include <stdint.h>

#include "rt_texture.h"

namespace rtd {

constexpr uint32_t kFeatureChannels = 8;        // albedo 0..2, normal 3..5, depth 6, coverage 7
constexpr uint32_t kFeatureNoId = 0xffffffffu;  // id of a sample that hit nothing

// The register form of one rt_material record (the same fields rt_shade.h load_material fills for the hit processing).
RT_DEV Mat feature_material(const rt_material& r) {
    Mat m;
    m.type = r.type; m.tex_type = r.tex_type; m.smoothness = r.smoothness; m.ior = r.ior;
    m.tiling = r.tiling;
    for (int c = 0; c < 3; ++c) {
        m.rgb0[c] = r.rgb0[c];
        m.rgb1[c] = r.rgb1[c];
    }
    m.luminance = r.luminance;
    return m;
}

// Emissive::Emit(Payload{}) of the sky material without its luminance: the texture at uv (0, 0) (material.cpp:172-175).
RT_DEV V3 feature_sky_albedo(const Mat& sky) { return eval_texture(sky, 0.f, 0.f); }

// One sample.  hit: the closest hit exists; then m = the hit sphere's material, origIdx its original index, t / nrm / (u, v) the
// hit record's distance, normal and texture coordinates.  sky: feature_sky_albedo of the scene's sky.
RT_DEV void feature_sample(bool hit, const Mat& m, uint32_t origIdx, float t, V3 nrm, float u, float v, V3 sky, float out[kFeatureChannels],
                           uint32_t& id) {
    if (!hit) {
        out[0] = sky.x; out[1] = sky.y; out[2] = sky.z;
        out[3] = 0.f; out[4] = 0.f; out[5] = 0.f;
        out[6] = 0.f;
        out[7] = 0.f;
        id = kFeatureNoId;
        return;
    }
    const V3 alb = m.type == RT_MAT_DIELECTRIC_TRANSPARENT ? v3(1.f, 1.f, 1.f) : eval_texture(m, u, v);
    out[0] = alb.x; out[1] = alb.y; out[2] = alb.z;
    out[3] = nrm.x; out[4] = nrm.y; out[5] = nrm.z;
    out[6] = t;
    out[7] = 1.f;
    id = origIdx;
}

}  // namespace rtd
