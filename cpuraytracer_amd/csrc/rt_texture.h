// rt_texture.h — the material record as the hit processing holds it, and Texture::Evaluate (texture.cpp:8-11, :20-33).
// Plain C++ over rt_device_math.h: compiled for the device (rt_shade.h, rt_kernels.h) and for the host (rt_features.h's host
// entry) from this one source.
#pragma once

#include <stdint.h>

#include "../../include/rt_api.h"
#include "rt_device_math.h"

namespace rtd {

// --------------------------------------------------------- textures (A14), getters (A13)
// Material record held in registers (loaded as three 16-byte reads; a by-value struct copy would
// be demoted to scratch/LDS by the compiler).
struct Mat {
    uint32_t type, tex_type;
    float smoothness, ior, tiling;
    float rgb0[3], rgb1[3];
    float luminance;
};
RT_DEV V3 eval_texture(const Mat& m, float u, float v) {
    if (m.tex_type == RT_TEX_CHECKER) {  // texture.cpp:20-33
        const int iu = (int)(m.tiling * u);
        const int iv = (int)(m.tiling * v);
        if (iu % 2 == iv % 2) return v3(m.rgb0[0], m.rgb0[1], m.rgb0[2]);
        return v3(m.rgb1[0], m.rgb1[1], m.rgb1[2]);
    }
    return v3(m.rgb0[0], m.rgb0[1], m.rgb0[2]);  // texture.cpp:8-11
}

}  // namespace rtd
