// rt_camera.hip -- rt_set_camera's one write to device memory (host/rt_camera_launch.h): the camera origin in the records of lights
// 1 .. (Shade's view direction, rt_shade.h).  A unit of its own, so that rt_capi.hip's and rt_denoise.hip's device code stay what they were.
#include <hip/hip_runtime.h>

#include "host/rt_camera_launch.h"
#include "rt_params.h"

namespace rtd {

// One thread per record; the origin by value.  Plain stores.
__global__ void __launch_bounds__(64) rt_light_camera_kernel(LightRec* __restrict__ recs, uint32_t n, float ox, float oy, float oz) {
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= n) return;
    recs[k].cam_o[0] = ox;
    recs[k].cam_o[1] = oy;
    recs[k].cam_o[2] = oz;
}

}  // namespace rtd

namespace rtcam {

int LaunchLightCamera(void* stream, rtd::LightRec* recs, uint32_t n, const float origin[3]) {
    if (n == 0u) return (int)hipSuccess;
    if (!recs) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rtd::rt_light_camera_kernel, dim3((n + 63u) / 64u), dim3(64), 0, static_cast<hipStream_t>(stream), recs, n, origin[0], origin[1],
                       origin[2]);
    return (int)hipGetLastError();
}

}  // namespace rtcam
