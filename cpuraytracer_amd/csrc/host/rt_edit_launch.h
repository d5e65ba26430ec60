// rt_edit_launch.h -- what rt_capi.hip sees of the edits' translation unit (rt_edit.hip): three launchers over plain pointers,
// and the host's way from a caller's list of ids to the set the forget kernel and its host twin test (../rt_forget.h).  The kernels
// live in a unit of their own for the denoiser's reason: one more kernel in rt_capi.hip changes the register allocation of the trace
// variants.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../../include/rt_api.h"
#include "../rt_forget.h"

namespace rtd {
struct LightRec;
}

namespace rtedit {

// sun_rad of lights 1 .. : at most RT_MAX_LIGHTS - 1 records, by value in the launch
struct LightRadiance {
    float rad[RT_MAX_LIGHTS - 1][3];
};

// Writes recs[k].sun_rad = R.rad[k] for k < n <= RT_MAX_LIGHTS - 1 on the stream: the one piece of device memory that holds a light's
// colour and luminance (rt_params.h LightRec; lights 1 .. of the scene's list -- the far-tier record behind them carries no radiance).
// The floats travel by value, so nothing the caller may overwrite is read later, and launches queued before it on the stream still
// read the old radiance.  n == 0: nothing is launched.  Returns the hipError_t of the launch as an int (0: launched).
int LaunchLightRadiance(void* stream, rtd::LightRec* recs, uint32_t n, const LightRadiance& R);

// Writes every field of recs[k] but cam_o from values[k] for k < n <= RT_MAX_LIGHTS on the stream (rt_turn_lights: direction, radiance,
// the shadow index's constants and its three table pointers, of lights 1 .. and of the far-tier record behind them).  values is host
// memory, read before the call returns: the records travel by value.  n == 0: nothing is launched.  Returns the hipError_t of the launch.
int LaunchLightIndex(void* stream, rtd::LightRec* recs, uint32_t n, const rtd::LightRec* values);

// Stores len[p] = 0 for every p < npix with forget_member(F, ids[p]) on the stream; every other word of len stays.  F.bits, where
// not null, is device memory that holds forget_table_words(F.n_bits) words by the time the kernel runs.  npix == 0: nothing is
// launched.  Returns the hipError_t of the launch as an int.
int LaunchTemporalForget(void* stream, uint32_t* len, const uint32_t* ids, uint32_t npix, const rtd::ForgetSet& F);

// A caller's list of ids as a set.  Ids at or above n_spheres (other than the sky's 0xffffffff) match nothing and are left out.  Up to
// kForgetInlineIds remaining ids: the inline form, table empty.  More: the table form, F.bits still NULL -- the caller points it at
// wherever the table's words lie (the host twin: at `table` itself; the device: at their copy).  nothing: no pixel can match.
struct ForgetPlan {
    rtd::ForgetSet set{};
    std::vector<uint32_t> table;
    bool nothing = true;
};
inline ForgetPlan PlanForget(const uint32_t* ids, uint32_t n_ids, uint32_t n_spheres) {
    ForgetPlan P;
    uint32_t kept = 0, top = 0;
    for (uint32_t k = 0; k < n_ids; ++k) {
        if (ids[k] == rtd::kForgetSkyId) P.set.sky = 1u;
        else if (ids[k] < n_spheres) ++kept, top = ids[k] > top ? ids[k] : top;
    }
    P.nothing = kept == 0u && P.set.sky == 0u;
    if (kept <= rtd::kForgetInlineIds) {
        for (uint32_t k = 0; k < n_ids; ++k)
            if (ids[k] != rtd::kForgetSkyId && ids[k] < n_spheres) P.set.ids[P.set.n_inline++] = ids[k];
        return P;
    }
    P.set.n_bits = top + 1u;
    P.table.assign(rtd::forget_table_words(P.set.n_bits), 0u);
    for (uint32_t k = 0; k < n_ids; ++k)
        if (ids[k] != rtd::kForgetSkyId && ids[k] < n_spheres) P.table[ids[k] >> 5] |= 1u << (ids[k] & 31u);
    return P;
}

}  // namespace rtedit
