// rt_forget_host.cpp -- rt_unit_temporal_forget_host: rt_temporal_forget's kernel on the host, from the same membership rule
// (../rt_forget.h) over the same set (rt_edit_launch.h PlanForget).  Plain C++ with no HIP header.  Needs no GPU.
#include <string>

#include "../../../include/rt_api.h"
#include "../rt_forget.h"
#include "rt_edit_launch.h"
#include "rt_error.h"

using rtprep::Fail;

extern "C" int rt_unit_temporal_forget_host(uint32_t* len, const uint32_t* ids, uint32_t npix, uint32_t n_spheres, const uint32_t* forget_ids, uint32_t n_ids) {
    const char* who = "rt_unit_temporal_forget_host";
    if (npix != 0u && (!len || !ids)) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null len or ids");
    if (n_ids != 0u && !forget_ids) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null forget_ids with n_ids > 0");
    rtedit::ForgetPlan P = rtedit::PlanForget(forget_ids, n_ids, n_spheres);
    if (P.nothing) return RT_OK;
    if (!P.table.empty()) P.set.bits = P.table.data();
    for (uint32_t p = 0; p < npix; ++p)
        if (rtd::forget_member(P.set, ids[p])) len[p] = 0u;
    return RT_OK;
}
