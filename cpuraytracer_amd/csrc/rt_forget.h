// rt_forget.h -- which pixels of the temporal history rt_temporal_forget empties: the membership rule, written once
// and compiled for the device (rt_edit.hip, rt_temporal_forget_kernel) and for the host (host/rt_temporal_host.cpp,
// rt_unit_temporal_forget_host).  Integers only: the two give the same words by construction.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_FORGET_FN __host__ __device__ __forceinline__
#else
#define RT_FORGET_FN inline
#endif

namespace rtd {

constexpr uint32_t kForgetSkyId = 0xffffffffu;  // the id a history pixel holds where the sample added last missed every sphere
constexpr uint32_t kForgetInlineIds = 16;       // up to this many ids travel by value in the launch; more go through a bitmask

// The set of ids to forget, in one of two forms.  Inline (bits == nullptr): the first n_inline words of ids.  Table: bit k of bits
// stands for sphere k < n_bits.  The sky is a flag of its own in both.  An id at or above the sphere count is in neither form:
// the host leaves it out when it builds the set.
struct ForgetSet {
    uint32_t ids[kForgetInlineIds];
    uint32_t n_inline;
    uint32_t n_bits;
    uint32_t sky;
    const uint32_t* bits;
};

RT_FORGET_FN bool forget_member(const ForgetSet& F, uint32_t id) {
    if (id == kForgetSkyId) return F.sky != 0u;
    if (F.bits) return id < F.n_bits && ((F.bits[id >> 5] >> (id & 31u)) & 1u) != 0u;
    bool hit = false;
    for (uint32_t k = 0; k < kForgetInlineIds; ++k) hit = hit || (k < F.n_inline && F.ids[k] == id);
    return hit;
}

// The words of a table over n_bits ids
RT_FORGET_FN uint32_t forget_table_words(uint32_t n_bits) { return (n_bits + 31u) / 32u; }

}  // namespace rtd
