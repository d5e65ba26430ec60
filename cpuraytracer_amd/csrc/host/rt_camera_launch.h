// rt_camera_launch.h -- what rt_capi.hip sees of the camera patch's translation unit (rt_camera.hip): one launcher over a plain
// pointer.  The kernel lives in a unit of its own for the denoiser's reason: one more kernel in rt_capi.hip changes the register
// allocation of the trace variants.
#pragma once

#include <stdint.h>

namespace rtd {
struct LightRec;
}

namespace rtcam {

// Writes recs[k].cam_o = origin for k < n on the stream: the one piece of device memory that holds the camera (rt_params.h LightRec;
// lights 1 .. of the scene's list).  The three floats travel by value in the launch, so nothing the caller may overwrite is read
// later, and launches queued before it on the stream still read the old origin.  n == 0: nothing is launched.
// Returns the hipError_t of the launch as an int (0: launched).
int LaunchLightCamera(void* stream, rtd::LightRec* recs, uint32_t n, const float origin[3]);

}  // namespace rtcam
