// rt_edit.hip -- the two writes to device memory of the shading edits that are not table copies (host/rt_edit_launch.h): the radiance
// in the records of lights 1 .. (rt_set_lights) and the forgotten pixels' history length (rt_temporal_forget).  A unit of its own, so
// that rt_capi.hip's and rt_denoise.hip's device code stay what they were.
#include <hip/hip_runtime.h>

#include "host/rt_edit_launch.h"
#include "rt_forget.h"
#include "rt_params.h"

namespace rtd {

// One thread per record; the radiances by value.  Plain stores.
__global__ void __launch_bounds__(64) rt_light_radiance_kernel(LightRec* __restrict__ recs, uint32_t n, rtedit::LightRadiance R) {
    const uint32_t k = threadIdx.x;
    if (k >= n || k >= (uint32_t)(RT_MAX_LIGHTS - 1)) return;
    // (a compile-time index into the by-value record: a run-time one would put the kernel arguments into scratch)
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)(RT_MAX_LIGHTS - 1); ++j)
        if (j == k) r0 = R.rad[j][0], r1 = R.rad[j][1], r2 = R.rad[j][2];
    recs[k].sun_rad[0] = r0;
    recs[k].sun_rad[1] = r1;
    recs[k].sun_rad[2] = r2;
}

// One thread per history pixel, consecutive pixels in consecutive lanes: one coalesced load of the ids, the membership test of
// rt_forget.h, one plain store where it holds.  No LDS, no atomics.
__global__ void __launch_bounds__(256) rt_temporal_forget_kernel(uint32_t* __restrict__ len, const uint32_t* __restrict__ ids, uint32_t npix, ForgetSet F) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    if (forget_member(F, ids[p])) len[p] = 0u;
}

}  // namespace rtd

namespace rtedit {

int LaunchLightRadiance(void* stream, rtd::LightRec* recs, uint32_t n, const LightRadiance& R) {
    if (n == 0u) return (int)hipSuccess;
    if (!recs || n > (uint32_t)(RT_MAX_LIGHTS - 1)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rtd::rt_light_radiance_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), recs, n, R);
    return (int)hipGetLastError();
}

int LaunchTemporalForget(void* stream, uint32_t* len, const uint32_t* ids, uint32_t npix, const rtd::ForgetSet& F) {
    if (npix == 0u) return (int)hipSuccess;
    if (!len || !ids) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rtd::rt_temporal_forget_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), len, ids, npix, F);
    return (int)hipGetLastError();
}

}  // namespace rtedit
