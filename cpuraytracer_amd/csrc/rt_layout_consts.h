// rt_layout_consts.h -- the constants the scene preparation on the host (host/rt_scene_prep.cpp) shares with the kernels that read
// its tables (rt_params.h, rt_scan.h).  Plain C++: no HIP header, so that the host unit builds without one.
#pragma once

#include <stdint.h>

namespace rtd {

constexpr uint32_t kMaxLevels = 6;  // levels of group bounds (4-ary): 128 * 4^5 groups at most
// K of the filter margins (units of eps * a * G; the host folds the same K into each bound): the matrix-core level needs
// 101*16 (exact-path rounding, amplified by the member offsets) + ~600 (split-bf16 operands); levels tested on the VALU
// in f32 need 101*16 + 30; a one-sphere bound (offset 0) needs 16 + 30.
constexpr float kMarginK = 4096.f, kMarginKValu = 2048.f, kMarginKLeaf = 64.f;

}  // namespace rtd
