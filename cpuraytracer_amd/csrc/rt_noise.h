// rt_noise.h -- per-pixel noise estimate of the accumulated image (DESIGN.md "Noise estimate").
//
// With rt_set_noise_estimate on, the accumulation keeps, next to the HDR strip hdr[pixel][c] = sum_s v_s[c], the strip of second
// moments sq[pixel][c] = sum_s RN(v_s[c]^2), both binary32 and both added in increasing s (rt_kernels.h
// rt_accumulate_moments_kernel).  From the two sums and the sample count n this file derives, per pixel, the standard error of
// the pixel MEAN: absolute (HDR units, the three channels' variances summed) and relative to the pixel's brightness.
//
// The arithmetic is the contract: binary64, only + - * / and comparisons in the order written below, then one rounding to
// binary32 and the path's correctly rounded binary32 square root (rt_device_math.h sqrt_rn; rt_unit_math op 7 proves it equals
// IEEE).  No binary64 square root.  The file is compiled with -ffp-contract=off for the device and for the host
// (rt_unit_noise_estimate_host), so the kernel, the host twin and a numpy restatement give the same bits.  A NaN (floor == 0 on
// a black pixel with no variance: 0 / 0) is reported as a NaN; its sign and payload are not part of the contract.
#pragma once

#include <stdint.h>

#include "rt_device_math.h"

namespace rtd {

constexpr uint32_t kNoiseMaxThresholds = 8;

struct NoiseThresholds {
    float t[kNoiseMaxThresholds];
    uint32_t n;
};

// hdr, sq: the pixel's three sums; n >= 2 samples in them.  out[0] = absolute, out[1] = relative standard error of the mean.
RT_DEV void noise_estimate(const float hdr[3], const float sq[3], uint32_t n, float floor, float out[2]) {
    const double N = (double)n, N1 = (double)(n - 1u);
    double mean[3], var[3];
    for (int c = 0; c < 3; ++c) {
        const double S = (double)hdr[c], Q = (double)sq[c];
        mean[c] = S / N;
        double v = (Q - S * mean[c]) / N1;  // (product and difference round separately: -ffp-contract=off)
        if (!(v > 0.0)) v = 0.0;            // binary32 sums may leave Q < S^2 / n; a NaN (inf - inf) is no variance either
        var[c] = v;
    }
    const double V = (var[0] + var[1]) + var[2];
    const double M = (mean[0] + mean[1]) + mean[2];
    const double abs2 = V / N;
    const double d = M + (double)floor;
    out[0] = sqrt_rn((float)abs2);
    out[1] = sqrt_rn((float)(abs2 / (d * d)));
}

// rel is +0 .. +inf or a NaN (never negative): finite values order like their bit patterns
RT_DEV bool noise_is_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
// a pixel counts for threshold t when rel > t; a non-finite rel counts for every threshold
RT_DEV bool noise_above(float rel, uint32_t bits, float t) { return !noise_is_finite(bits) || rel > t; }

}  // namespace rtd
