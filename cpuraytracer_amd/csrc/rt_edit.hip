// rt_edit.hip -- the writes to device memory of the edits that are not table copies (host/rt_edit_launch.h): the radiance in the
// records of lights 1 .. (rt_set_lights), those records whole but for cam_o, with the far tier's (rt_turn_lights), and the forgotten
// pixels' history length (rt_temporal_forget).  A unit of its own, so that rt_capi.hip's and rt_denoise.hip's device code stay what
// they were.
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

// rt_turn_lights: direction, radiance and shadow index of the records of lights 1 .. and of the far-tier record behind them -- every
// field but cam_o, which a turn leaves alone.  One thread per record, the records by value, plain stores.
struct LightIndexRecs {
    LightRec rec[RT_MAX_LIGHTS];
};
__global__ void __launch_bounds__(64) rt_light_index_kernel(LightRec* __restrict__ recs, uint32_t n, LightIndexRecs R) {
    const uint32_t k = threadIdx.x;
    if (k >= n || k >= (uint32_t)RT_MAX_LIGHTS) return;
    // (compile-time indices into the by-value records, as above)
    LightRec r = R.rec[0];
#pragma unroll
    for (uint32_t j = 1; j < (uint32_t)RT_MAX_LIGHTS; ++j)
        if (j == k) r = R.rec[j];
    LightRec& d = recs[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        d.sun_dir[c] = r.sun_dir[c];
        d.sun_rad[c] = r.sun_rad[c];
        d.sg_e1[c] = r.sg_e1[c];
        d.sg_e2[c] = r.sg_e2[c];
    }
    d.sg_u0 = r.sg_u0, d.sg_v0 = r.sg_v0, d.sg_inv_cell = r.sg_inv_cell, d.sg_p0sq = r.sg_p0sq;
    d.sg_nx = r.sg_nx, d.sg_ny = r.sg_ny, d.sg_nglobal = r.sg_nglobal, d.sg_enabled = r.sg_enabled;
    d.cell_start = r.cell_start, d.entries = r.entries, d.global = r.global;
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

int LaunchLightIndex(void* stream, rtd::LightRec* recs, uint32_t n, const rtd::LightRec* values) {
    if (n == 0u) return (int)hipSuccess;
    if (!recs || !values || n > (uint32_t)RT_MAX_LIGHTS) return (int)hipErrorInvalidValue;
    rtd::LightIndexRecs R{};
    for (uint32_t k = 0; k < n; ++k) R.rec[k] = values[k];
    hipLaunchKernelGGL(rtd::rt_light_index_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), recs, n, R);
    return (int)hipGetLastError();
}

int LaunchTemporalForget(void* stream, uint32_t* len, const uint32_t* ids, uint32_t npix, const rtd::ForgetSet& F) {
    if (npix == 0u) return (int)hipSuccess;
    if (!len || !ids) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rtd::rt_temporal_forget_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream), len, ids, npix, F);
    return (int)hipGetLastError();
}

}  // namespace rtedit
