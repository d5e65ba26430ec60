// rt_denoise.h -- feature-guided a-trous filter of the accumulated picture (DESIGN.md "Denoise").
//
// The filter reads four strips the context owns -- hdr and sq (rt_noise.h) after n >= 2 samples, the feature sums (rt_features.h)
// after m >= 1 samples -- and writes strips of its own.  This file is the only place its arithmetic is written: binary32, only
// + - * / and comparisons in the order and association below, the one square root inside noise_estimate.  It is compiled with
// -ffp-contract=off for the device (rt_denoise.hip) and for the host (host/rt_denoise_host.cpp, rt_unit_denoise_host), so the
// kernels, the host twin and a numpy restatement give the same bits.  Pixels whose inputs are all finite are covered; a NaN's
// sign and payload are not.  Where the picture has no usable second moments -- one sample per pixel, the noise estimate off -- v0 comes
// from the picture's own neighbourhoods instead ("the spatial variance source" below); everything after v0 is the same.
#pragma once

#include <stdint.h>

#include "rt_noise.h"

namespace rtd {

constexpr uint32_t kDenoiseMaxLevels = 5;

// rt_denoise_params of include/rt_api.h, field for field
struct DenoiseParams {
    uint32_t levels;
    float k_normal, k_depth, k_albedo, k_coverage, k_colour, var_floor;
};

// The filter's state of a pixel: mean colour and the variance of that mean (channels summed).
struct DenoiseState {
    float c[3];
    float v;
};

// Per pixel, once: c0 = hdr / n, v0 = sigma^2 with sigma the absolute standard error of rt_noise.h (floor 0), g = feat / m.
RT_DEV void denoise_prepare(const float hdr[3], const float sq[3], uint32_t n, const float feat[8], uint32_t m, DenoiseState& s, float g[8]) {
    const float fn = (float)n, fm = (float)m;
    for (int k = 0; k < 3; ++k) s.c[k] = hdr[k] / fn;
    float est[2];
    noise_estimate(hdr, sq, n, 0.0f, est);
    s.v = est[0] * est[0];
    for (int k = 0; k < 8; ++k) g[k] = feat[k] / fm;
}

// B3 spline {1/16, 1/4, 3/8, 1/4, 1/16}: every value and every product of two is exact in binary32
RT_DEV float denoise_h(int a) { return a == 2 ? 0.375f : ((a == 1 || a == 3) ? 0.25f : 0.0625f); }

struct DenoiseSums {
    float sc[3];
    float sv, sw;
};

RT_DEV void denoise_begin(DenoiseSums& S) {
    S.sc[0] = S.sc[1] = S.sc[2] = 0.0f;
    S.sv = 0.0f;
    S.sw = 0.0f;
}

// One tap q of pixel p: hab = h[a] * h[b]; (sp, gp) the centre's state and guides, (sq, gq) the tap's.
RT_DEV void denoise_tap(const DenoiseParams& P, float hab, const DenoiseState& sp, const float gp[8], const DenoiseState& sq, const float gq[8],
                        DenoiseSums& S) {
    const float dn0 = gp[3] - gq[3], dn1 = gp[4] - gq[4], dn2 = gp[5] - gq[5];
    const float xn = P.k_normal * ((dn0 * dn0 + dn1 * dn1) + dn2 * dn2);
    const float da0 = gp[0] - gq[0], da1 = gp[1] - gq[1], da2 = gp[2] - gq[2];
    const float xa = P.k_albedo * ((da0 * da0 + da1 * da1) + da2 * da2);
    const float dz = gp[6] - gq[6];
    const float zm = gp[6] > gq[6] ? gp[6] : gq[6];
    const float xz = P.k_depth * ((dz * dz) / (zm * zm + 1e-12f));
    const float dc = gp[7] - gq[7];
    const float xc = P.k_coverage * (dc * dc);
    const float dl0 = sp.c[0] - sq.c[0], dl1 = sp.c[1] - sq.c[1], dl2 = sp.c[2] - sq.c[2];
    const float xl = P.k_colour * (((dl0 * dl0 + dl1 * dl1) + dl2 * dl2) / ((sp.v + sq.v) + P.var_floor));
    const float x = (((xn + xz) + xa) + xc) + xl;
    const float ww = hab / (1.0f + x);
    for (int k = 0; k < 3; ++k) S.sc[k] = S.sc[k] + ww * sq.c[k];
    S.sv = S.sv + (ww * ww) * sq.v;
    S.sw = S.sw + ww;
}

// After the 25 taps (the centre tap has x == 0, so sw >= 9/64)
RT_DEV void denoise_finish(const DenoiseSums& S, DenoiseState& out) {
    for (int k = 0; k < 3; ++k) out.c[k] = S.sc[k] / S.sw;
    out.v = S.sv / (S.sw * S.sw);
}

// ---- the spatial variance source: where a pixel has too few samples for a variance of its own (n = 1 has none), v0 is
// the guide-weighted variance of c0 over the (2R+1)^2 window around it.  sq is not read; c0 and g are denoise_prepare's.
constexpr uint32_t kVarianceMoments = 0, kVarianceSpatial = 1;  // rt_variance_params::source
constexpr uint32_t kVarianceMaxRadius = 3;

// rt_variance_params of include/rt_api.h, field for field
struct VarianceParams {
    uint32_t source, radius;
};

RT_DEV bool variance_params_ok(const VarianceParams& V) {
    if (V.source == kVarianceMoments) return true;  // (the radius is read only under the spatial source)
    return V.source == kVarianceSpatial && V.radius >= 1u && V.radius <= kVarianceMaxRadius;
}

// c0 and g alone: denoise_prepare's two quotients without its noise estimate
RT_DEV void denoise_prepare_mean(const float hdr[3], uint32_t n, const float feat[8], uint32_t m, float c[3], float g[8]) {
    const float fn = (float)n, fm = (float)m;
    for (int k = 0; k < 3; ++k) c[k] = hdr[k] / fn;
    for (int k = 0; k < 8; ++k) g[k] = feat[k] / fm;
}

struct SpatialSums {
    float s1[3], s2[3];
    float sw;
};

RT_DEV void spatial_begin(SpatialSums& S) {
    for (int k = 0; k < 3; ++k) S.s1[k] = S.s2[k] = 0.0f;
    S.sw = 0.0f;
}

// One tap q of pixel p: the four guide terms are denoise_tap's, expression for expression; there is no colour term and no h.
RT_DEV void spatial_tap(const DenoiseParams& P, const float gp[8], const float cq[3], const float gq[8], SpatialSums& S) {
    const float dn0 = gp[3] - gq[3], dn1 = gp[4] - gq[4], dn2 = gp[5] - gq[5];
    const float xn = P.k_normal * ((dn0 * dn0 + dn1 * dn1) + dn2 * dn2);
    const float da0 = gp[0] - gq[0], da1 = gp[1] - gq[1], da2 = gp[2] - gq[2];
    const float xa = P.k_albedo * ((da0 * da0 + da1 * da1) + da2 * da2);
    const float dz = gp[6] - gq[6];
    const float zm = gp[6] > gq[6] ? gp[6] : gq[6];
    const float xz = P.k_depth * ((dz * dz) / (zm * zm + 1e-12f));
    const float dc = gp[7] - gq[7];
    const float xc = P.k_coverage * (dc * dc);
    const float x = ((xn + xz) + xa) + xc;
    const float w = 1.0f / (1.0f + x);
    for (int k = 0; k < 3; ++k) {
        S.s1[k] = S.s1[k] + w * cq[k];
        S.s2[k] = S.s2[k] + w * (cq[k] * cq[k]);
    }
    S.sw = S.sw + w;
}

// After the taps (the centre tap has w == 1, so sw >= 1): the weighted variance per channel, floor 0, channels summed
RT_DEV float spatial_finish(const SpatialSums& S) {
    float d[3];
    for (int k = 0; k < 3; ++k) {
        const float mu = S.s1[k] / S.sw, e = S.s2[k] / S.sw;
        d[k] = e - mu * mu;
        if (!(d[k] > 0.0f)) d[k] = 0.0f;
    }
    return (d[0] + d[1]) + d[2];
}

// levels 1..5; every k and var_floor finite and >= 0, var_floor > 0
RT_DEV bool denoise_params_ok(const DenoiseParams& P) {
    const float k[6] = {P.k_normal, P.k_depth, P.k_albedo, P.k_coverage, P.k_colour, P.var_floor};
    for (int i = 0; i < 6; ++i)
        if (!(k[i] >= 0.0f) || !(k[i] <= 3.402823466e38f)) return false;
    return P.levels >= 1u && P.levels <= kDenoiseMaxLevels && P.var_floor > 0.0f;
}

}  // namespace rtd
