// rt_trace_variants.h -- the ONE list of the kernel variants librt_hip.so instantiates.  rt_capi.hip expands it into its launch
// tables (tuple -> &rt_trace_kernel<...>, &rt_trace_kernel_lights<...>), host/launch_plan_selftest.cpp and the launch plan's unit
// entry into the same tuples without a kernel behind them.  Plain C++: no HIP header.
//
// A row is X(kLds, kThreads, kScan, kCache, kHitLds, kCarry, kStash, kMatsL2, kSgLds, kGridQ), the template arguments of
// rt_trace_kernel (rt_kernels.h) in their order.  Every row exists twice in the library: for scenes with one light, and as the
// _lights twin.  55 rows; the order is the order of instantiation and so the order of the kernels in the code object.  Three of the
// rows exist once more without far-hit state (RT_TRACE_LEAN_VARIANTS below), instantiated behind the 110.
#pragma once

#include <stdint.h>

// workgroup size T of a scan without hit stash: path cache on / off, times the hit-processing tables (flat scan) or the
// hierarchy's bounds (hierarchy scan) provably in LDS or not
#define RT_TRACE_PLAIN4(X, LDS, T, M)                            \
    X(LDS, T, M, true, true, false, false, false, false, false)  \
    X(LDS, T, M, false, true, false, false, false, false, false) \
    RT_TRACE_PLAIN2(X, LDS, T, M)
// ... and of a scan that has no such tables (VALU scan; cell grid below 1024 threads): path cache on / off
#define RT_TRACE_PLAIN2(X, LDS, T, M)                            \
    X(LDS, T, M, true, false, false, false, false, false, false) \
    X(LDS, T, M, false, false, false, false, false, false, false)
#define RT_TRACE_SIZES(FAMILY, X, LDS, M) FAMILY(X, LDS, 1024, M) FAMILY(X, LDS, 512, M) FAMILY(X, LDS, 256, M)

#define RT_TRACE_VARIANTS(X)                                                                                                    \
    /* frame pipelining: the flat LDS scan that carries its unfinished paths */                                                 \
    X(true, 1024, 1, true, true, true, false, false, false, false)                                                              \
    /* cell grid, every table in LDS: hit stash, path cache, neither */                                                         \
    X(true, 1024, 3, true, true, false, true, false, false, false)                                                              \
    X(true, 1024, 3, true, true, false, false, false, false, false)                                                             \
    X(true, 1024, 3, false, true, false, false, false, false, false)                                                            \
    /* cell grid, tables in global memory, hit stash: with the shadow index in LDS, with the quantised bounds in LDS, plain */    \
    X(false, 1024, 3, true, true, false, true, false, true, false)                                                              \
    X(false, 1024, 3, true, true, false, true, false, false, true)                                                              \
    X(false, 1024, 3, true, true, false, true, false, false, false)                                                             \
    /* ... without the stash: cells in LDS with and without path cache, cells in global memory */                               \
    X(false, 1024, 3, true, true, false, false, false, false, false)                                                            \
    X(false, 1024, 3, false, true, false, false, false, false, false)                                                           \
    X(false, 1024, 3, false, false, false, false, false, false, false)                                                          \
    /* ... and in smaller workgroups (cells in global memory) */                                                                \
    X(false, 512, 3, false, false, false, false, false, false, false)                                                           \
    X(false, 512, 3, true, false, false, false, false, false, false)                                                            \
    X(false, 256, 3, false, false, false, false, false, false, false)                                                           \
    X(false, 256, 3, true, false, false, false, false, false, false)                                                            \
    /* hit stash over the hierarchy scan: bounds in LDS or not */                                                               \
    X(false, 1024, 2, true, true, false, true, false, false, false)                                                             \
    X(false, 1024, 2, true, false, false, true, false, false, false)                                                            \
    /* hit stash over the flat scan: materials through L2, hit-processing tables in LDS, not all of them in LDS */              \
    X(true, 1024, 1, true, true, false, true, true, false, false)                                                               \
    X(true, 1024, 1, true, true, false, true, false, false, false)                                                              \
    X(true, 1024, 1, true, false, false, true, false, false, false)                                                             \
    /* no stash: hierarchy, flat, VALU scan with LDS tables, VALU scan with global tables */                                    \
    RT_TRACE_SIZES(RT_TRACE_PLAIN4, X, false, 2)                                                                                \
    RT_TRACE_SIZES(RT_TRACE_PLAIN4, X, true, 1)                                                                                 \
    RT_TRACE_SIZES(RT_TRACE_PLAIN2, X, true, 0)                                                                                 \
    RT_TRACE_SIZES(RT_TRACE_PLAIN2, X, false, 0)

// The scans of the unit kernels k_unit_closest and rt_features_kernel, X(kLds, kScan): cell grid, hierarchy, flat, VALU scan with
// LDS tables, VALU scan with global tables.
#define RT_SCAN_VARIANTS(X) X(false, 3) X(false, 2) X(true, 1) X(true, 0) X(false, 0)

// The rows of RT_TRACE_VARIANTS that exist a second time WITHOUT far-hit state (rt_kernels.h trace_body, kFarState == false:
// rt_trace_kernel_lean and rt_trace_kernel_lights_lean): the flat LDS hit-stash family -- kLds, kScan == 1, kStash, no frame
// pipelining; the stash exists at 1024 threads only.  Same tuples, same kernel words: a lean kernel is its row's kernel for picture
// launches (host/rt_launch_plan.h FarStateLean), not another row, and the launcher reports which of the two ran beside the plan
// (rt_unit_last_trace_far_state).  Six more functions in the library, behind the 110.
#define RT_TRACE_LEAN_VARIANTS(X)                                  \
    X(true, 1024, 1, true, true, false, true, true, false, false)  \
    X(true, 1024, 1, true, true, false, true, false, false, false) \
    X(true, 1024, 1, true, false, false, true, false, false, false)

namespace rtplan {

// Which rt_trace_kernel: `lights` picks the _lights twin, the rest are the template arguments.
struct TraceKernelId {
    bool lights, kLds;
    int kThreads, kScan;
    bool kCache, kHitLds, kCarry, kStash, kMatsL2, kSgLds, kGridQ;
};
struct ScanKernelId {
    bool kLds;
    int kScan;
};

// same template arguments (`lights` is not one of them: every row has both twins)
constexpr bool SameVariant(const TraceKernelId& a, const TraceKernelId& b) {
    return a.kLds == b.kLds && a.kThreads == b.kThreads && a.kScan == b.kScan && a.kCache == b.kCache && a.kHitLds == b.kHitLds &&
           a.kCarry == b.kCarry && a.kStash == b.kStash && a.kMatsL2 == b.kMatsL2 && a.kSgLds == b.kSgLds && a.kGridQ == b.kGridQ;
}

#define RT_VARIANT_ID(LDS, T, M, CACHE, HIT, CARRY, STASH, ML2, SG, GQ) {false, LDS, T, M, CACHE, HIT, CARRY, STASH, ML2, SG, GQ},
constexpr TraceKernelId kTraceVariants[] = {RT_TRACE_VARIANTS(RT_VARIANT_ID)};
#undef RT_VARIANT_ID
constexpr int kTraceVariantCount = (int)(sizeof(kTraceVariants) / sizeof(kTraceVariants[0]));
static_assert(kTraceVariantCount == 55, "55 variants of rt_trace_kernel, each with its _lights twin");

#define RT_VARIANT_ID(LDS, T, M, CACHE, HIT, CARRY, STASH, ML2, SG, GQ) {false, LDS, T, M, CACHE, HIT, CARRY, STASH, ML2, SG, GQ},
constexpr TraceKernelId kTraceLeanVariants[] = {RT_TRACE_LEAN_VARIANTS(RT_VARIANT_ID)};
#undef RT_VARIANT_ID
constexpr int kTraceLeanVariantCount = (int)(sizeof(kTraceLeanVariants) / sizeof(kTraceLeanVariants[0]));
// position of the variant in the lean list, or -1: it exists with far-hit state only
constexpr int FindLeanVariant(const TraceKernelId& id) {
    for (int i = 0; i < kTraceLeanVariantCount; ++i)
        if (SameVariant(kTraceLeanVariants[i], id)) return i;
    return -1;
}
// the lean list names exactly the flat LDS hit-stash rows without frame pipelining, each of them a row of the list above
constexpr bool LeanFamily(const TraceKernelId& k) { return k.kLds && k.kScan == 1 && k.kStash && !k.kCarry; }
constexpr bool LeanListIsTheFamily() {
    int family = 0;
    for (int i = 0; i < kTraceVariantCount; ++i) {
        if (LeanFamily(kTraceVariants[i]) != (FindLeanVariant(kTraceVariants[i]) >= 0)) return false;
        family += LeanFamily(kTraceVariants[i]) ? 1 : 0;
    }
    return family == kTraceLeanVariantCount;
}
static_assert(LeanListIsTheFamily(), "RT_TRACE_LEAN_VARIANTS: the flat LDS hit-stash rows of RT_TRACE_VARIANTS, no more and no fewer");

#define RT_SCAN_ID(LDS, M) {LDS, M},
constexpr ScanKernelId kScanVariants[] = {RT_SCAN_VARIANTS(RT_SCAN_ID)};
#undef RT_SCAN_ID
constexpr int kScanVariantCount = (int)(sizeof(kScanVariants) / sizeof(kScanVariants[0]));

// row of the variant in the list, or -1: not instantiated
constexpr int FindTraceVariant(const TraceKernelId& id) {
    for (int i = 0; i < kTraceVariantCount; ++i)
        if (SameVariant(kTraceVariants[i], id)) return i;
    return -1;
}
constexpr int FindScanVariant(const ScanKernelId& id) {
    for (int i = 0; i < kScanVariantCount; ++i)
        if (kScanVariants[i].kLds == id.kLds && kScanVariants[i].kScan == id.kScan) return i;
    return -1;
}

}  // namespace rtplan
