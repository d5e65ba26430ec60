// rt_temporal.h -- temporal accumulation for the denoiser (DESIGN.md "Temporal accumulation"): reproject the previous frame's
// pre-filter state into the current camera, validate it against the guides, blend colour and variance.
//
// This file is the only place that arithmetic is written: binary32, only + - * / and comparisons in the order and association
// below, dot(a, b) = (a0*b0 + a1*b1) + a2*b2, the correctly rounded division and square root (rt_device_math.h sqrt_rn).  It is
// compiled with -ffp-contract=off for the device (rt_denoise.hip) and for the host (host/rt_temporal_host.cpp,
// rt_unit_temporal_host), so the kernel, the host twin and a numpy restatement give the same bits.  A NaN anywhere rejects the
// pixel: every test is written as "reject unless".
#pragma once

#include <stdint.h>

#include "rt_denoise.h"

namespace rtd {

constexpr uint32_t kTemporalMaxHistory = 64;
constexpr uint32_t kTemporalNoTarget = 0xffffffffu;
// (float)W and (float)(first_row + num_rows) must be exact for "fx < W" to bound (uint32)fx
constexpr uint32_t kTemporalMaxSide = 1u << 24;

// rt_temporal_params of include/rt_api.h, field for field
struct TemporalParams {
    uint32_t max_history, use_id;
    float depth_tol, normal_tol, coverage_tol;
};

// What the reprojection reads of a camera record: origin, x, y and w = origin_image_plane - origin.
struct TemporalCam {
    float o[3], x[3], y[3], w[3];
};

// The picture and the strip's rows of it: image row y = first_row + local row.
struct TemporalGeom {
    uint32_t W, H, first_row, num_rows;
};

RT_DEV float temporal_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RT_DEV void temporal_cam(const float origin[3], const float x[3], const float y[3], const float origin_image_plane[3], TemporalCam& C) {
    for (int k = 0; k < 3; ++k) {
        C.o[k] = origin[k];
        C.x[k] = x[k];
        C.y[k] = y[k];
        C.w[k] = origin_image_plane[k] - origin[k];
    }
}

// Where pixel (x, y) of camera C, at the depth its guides g give it, lies in the picture of camera Cp.  false: behind Cp or outside
// the strip.  true: (xi, yi) is the pixel of Cp's picture that contains the point, 0 <= xi < W and first_row <= yi < first_row +
// num_rows, and dist the point's distance from Cp's origin (hit pixels only; a sky pixel is reprojected by its direction).
RT_DEV bool temporal_reproject(const TemporalGeom& G, const TemporalCam& C, const TemporalCam& Cp, uint32_t x, uint32_t y, const float g[8], uint32_t& xi,
                               uint32_t& yi, float& dist) {
    const float u = ((float)x + 0.5f) / (float)G.W, vv = ((float)y + 0.5f) / (float)G.H;
    const float nx = 2.f * u - 1.f, ny = -2.f * vv + 1.f;
    float d[3], q[3];
    for (int k = 0; k < 3; ++k) d[k] = (C.w[k] + nx * C.x[k]) + ny * C.y[k];
    const float cov = g[7];
    dist = 0.f;
    if (cov > 0.f) {
        const float z = g[6] / cov;
        const float s = z / sqrt_rn(temporal_dot(d, d));
        for (int k = 0; k < 3; ++k) {
            const float P = C.o[k] + s * d[k];
            q[k] = P - Cp.o[k];
        }
        dist = sqrt_rn(temporal_dot(q, q));
    } else {
        for (int k = 0; k < 3; ++k) q[k] = d[k];
    }
    const float zw = temporal_dot(q, Cp.w) / temporal_dot(Cp.w, Cp.w);
    if (!(zw > 0.f)) return false;
    const float px = (temporal_dot(q, Cp.x) / temporal_dot(Cp.x, Cp.x)) / zw;
    const float py = (temporal_dot(q, Cp.y) / temporal_dot(Cp.y, Cp.y)) / zw;
    const float fx = ((px + 1.f) * 0.5f) * (float)G.W;
    const float fy = ((1.f - py) * 0.5f) * (float)G.H;
    if (!(fx >= 0.f && fx < (float)G.W)) return false;
    if (!(fy >= (float)G.first_row && fy < (float)(G.first_row + G.num_rows))) return false;
    xi = (uint32_t)fx;
    yi = (uint32_t)fy;
    return true;
}

// The current pixel (guides g, id, distance dist from the history's camera) against the history's pixel it fell into.
RT_DEV bool temporal_validate(const TemporalParams& T, const float g[8], uint32_t id, float dist, const float gh[8], uint32_t idh, uint32_t lenh) {
    if (!(lenh >= 1u)) return false;
    if (T.use_id != 0u && !(id == idh)) return false;
    const float cov = g[7];
    const float dc = cov - gh[7];
    const float adc = dc < 0.f ? -dc : dc;
    if (!(adc <= T.coverage_tol)) return false;
    const float dn[3] = {g[3] - gh[3], g[4] - gh[4], g[5] - gh[5]};
    if (!(temporal_dot(dn, dn) <= T.normal_tol)) return false;
    if (cov > 0.f) {
        if (!(gh[7] > 0.f)) return false;
        const float zh = gh[6] / gh[7];
        const float dz = dist - zh;
        const float zm = dist > zh ? dist : zh;
        if (!(dz * dz <= (T.depth_tol * T.depth_tol) * (zm * zm))) return false;
    } else if (!(cov == 0.f && gh[7] == 0.f)) {
        return false;
    }
    return true;
}

// s: the pixel's prepared state in, the blended state out.  sh, lenh: the history's, read only when accepted.  Returns len'.
RT_DEV uint32_t temporal_blend(const TemporalParams& T, bool accepted, DenoiseState& s, const DenoiseState& sh, uint32_t lenh) {
    if (!accepted) return 1u;
    const uint32_t cap = T.max_history - 1u;
    const uint32_t l = lenh < cap ? lenh : cap;
    const float L = (float)l;
    const float a = 1.f / (L + 1.f);
    const float b = 1.f - a;
    for (int k = 0; k < 3; ++k) s.c[k] = a * s.c[k] + b * sh.c[k];
    s.v = (a * a) * s.v + (b * b) * sh.v;
    return l + 1u;
}

// ---- the bilinear fetch (RT_TEMPORAL_FETCH_BILINEAR): the history is read at the four pixels whose centres surround the reprojected
// point instead of the one pixel that contains it.  Everything above is used as it stands.
constexpr uint32_t kTemporalFetchNearest = 1, kTemporalFetchBilinear = 4;

RT_DEV bool temporal_fetch_ok(uint32_t fetch) { return fetch == kTemporalFetchNearest || fetch == kTemporalFetchBilinear; }

// temporal_reproject that also yields the point itself, (fx, fy) in pixel units of Cp's picture: the same operations in the same order
// (kept beside it, not merged into it: the nearest fetch's code stays what it was), so xi, yi, dist and the refusals are its bits.
RT_DEV bool temporal_reproject_point(const TemporalGeom& G, const TemporalCam& C, const TemporalCam& Cp, uint32_t x, uint32_t y, const float g[8], float& fx,
                                     float& fy, uint32_t& xi, uint32_t& yi, float& dist) {
    const float u = ((float)x + 0.5f) / (float)G.W, vv = ((float)y + 0.5f) / (float)G.H;
    const float nx = 2.f * u - 1.f, ny = -2.f * vv + 1.f;
    float d[3], q[3];
    for (int k = 0; k < 3; ++k) d[k] = (C.w[k] + nx * C.x[k]) + ny * C.y[k];
    const float cov = g[7];
    dist = 0.f;
    if (cov > 0.f) {
        const float z = g[6] / cov;
        const float s = z / sqrt_rn(temporal_dot(d, d));
        for (int k = 0; k < 3; ++k) {
            const float P = C.o[k] + s * d[k];
            q[k] = P - Cp.o[k];
        }
        dist = sqrt_rn(temporal_dot(q, q));
    } else {
        for (int k = 0; k < 3; ++k) q[k] = d[k];
    }
    const float zw = temporal_dot(q, Cp.w) / temporal_dot(Cp.w, Cp.w);
    if (!(zw > 0.f)) return false;
    const float px = (temporal_dot(q, Cp.x) / temporal_dot(Cp.x, Cp.x)) / zw;
    const float py = (temporal_dot(q, Cp.y) / temporal_dot(Cp.y, Cp.y)) / zw;
    fx = ((px + 1.f) * 0.5f) * (float)G.W;
    fy = ((1.f - py) * 0.5f) * (float)G.H;
    if (!(fx >= 0.f && fx < (float)G.W)) return false;
    if (!(fy >= (float)G.first_row && fy < (float)(G.first_row + G.num_rows))) return false;
    xi = (uint32_t)fx;
    yi = (uint32_t)fy;
    return true;
}

// The four taps of an accepted point: pixel centres lie at +0.5, so the point lies between the centres of columns x0 and x0 + 1, tx of
// the way from the first to the second (0 <= tx <= 1: rx + 0.5f may round up to 1, and that tap (0, .) then weighs 0); rows likewise.  x0 = -1 where the point lies left of column 0's centre and y0 =
// first_row - 1 above the strip's first centre: those taps are outside.  (fx - (float)xi is exact: xi <= fx < xi + 1 < 2^24.)
struct TemporalTaps {
    int32_t x0, y0;  // column and IMAGE row of tap (0, 0)
    float tx, ty;
};

RT_DEV void temporal_taps(float fx, float fy, uint32_t xi, uint32_t yi, TemporalTaps& B) {
    const float rx = fx - (float)xi, ry = fy - (float)yi;
    if (rx >= 0.5f) {
        B.x0 = (int32_t)xi;
        B.tx = rx - 0.5f;
    } else {
        B.x0 = (int32_t)xi - 1;
        B.tx = rx + 0.5f;
    }
    if (ry >= 0.5f) {
        B.y0 = (int32_t)yi;
        B.ty = ry - 0.5f;
    } else {
        B.y0 = (int32_t)yi - 1;
        B.ty = ry + 0.5f;
    }
}

// Tap k = 0..3 is (i, j) = (k & 1, k >> 1): (0,0) (1,0) (0,1) (1,1).
RT_DEV float temporal_tap_weight(const TemporalTaps& B, int k) {
    const float wx = (k & 1) ? B.tx : 1.f - B.tx;
    const float wy = (k >> 1) ? B.ty : 1.f - B.ty;
    return wx * wy;
}

// Whether tap k lies inside the strip, and then its index q = (qy - first_row)*W + qx in the history's arrays.
RT_DEV bool temporal_tap_index(const TemporalGeom& G, const TemporalTaps& B, int k, uint32_t& q) {
    const int32_t qx = B.x0 + (k & 1), qy = B.y0 + (k >> 1);
    if (!(qx >= 0 && (uint32_t)qx < G.W)) return false;
    if (!(qy >= (int32_t)G.first_row && (uint32_t)qy < G.first_row + G.num_rows)) return false;
    q = ((uint32_t)qy - G.first_row) * G.W + (uint32_t)qx;
    return true;
}

// The sums over the taps that take part: inside the strip, w > 0 and temporal_validate -- the caller's business, tap by tap.  A tap
// that does not take part is never added, so nothing of it (an Inf, a NaN) reaches the result.
struct TemporalGather {
    float sc[3], sv, sw, wbest;
    uint32_t lmin, target;
};

RT_DEV void temporal_gather_begin(TemporalGather& S) {
    S.sc[0] = S.sc[1] = S.sc[2] = 0.f;
    S.sv = 0.f;
    S.sw = 0.f;
    S.wbest = 0.f;
    S.lmin = 0xffffffffu;
    S.target = kTemporalNoTarget;
}

// (w > 0 for every tap that gets here, so the first makes itself the target; later ones only with a strictly greater weight)
RT_DEV void temporal_gather_tap(TemporalGather& S, float w, const DenoiseState& sh, uint32_t lenh, uint32_t q) {
    for (int k = 0; k < 3; ++k) S.sc[k] = S.sc[k] + w * sh.c[k];
    S.sv = S.sv + (w * w) * sh.v;
    S.sw = S.sw + w;
    S.lmin = lenh < S.lmin ? lenh : S.lmin;
    if (w > S.wbest) {
        S.wbest = w;
        S.target = q;
    }
}

// false: no tap took part (rejected).  true: the history's value at the point -- colour sum(w c)/sw, variance sum(w^2 v)/sw^2 (the
// a-trous's convention, rt_denoise.h denoise_finish), length the shortest of the taps -- for the unchanged temporal_blend.
RT_DEV bool temporal_gather_finish(const TemporalGather& S, DenoiseState& sh, uint32_t& lenh) {
    if (!(S.sw > 0.f)) return false;
    for (int k = 0; k < 3; ++k) sh.c[k] = S.sc[k] / S.sw;
    sh.v = S.sv / (S.sw * S.sw);
    lenh = S.lmin;
    return true;
}

// max_history 1..64; every tolerance finite and >= 0
RT_DEV bool temporal_params_ok(const TemporalParams& T) {
    const float t[3] = {T.depth_tol, T.normal_tol, T.coverage_tol};
    for (int i = 0; i < 3; ++i)
        if (!(t[i] >= 0.0f) || !(t[i] <= 3.402823466e38f)) return false;
    return T.max_history >= 1u && T.max_history <= kTemporalMaxHistory;
}

RT_DEV bool temporal_geom_ok(const TemporalGeom& G) {
    return G.W >= 1u && G.H >= 1u && G.num_rows >= 1u && G.W <= kTemporalMaxSide && G.H <= kTemporalMaxSide && G.first_row <= kTemporalMaxSide &&
           G.num_rows <= kTemporalMaxSide - G.first_row;
}

}  // namespace rtd
