// rt_denoise_host.h -- what the host twins share (rt_denoise_host.cpp, rt_temporal_host.cpp): the levels of the filter over a
// prepared state, and the temporal parameters' check.  Host C++ only.
#pragma once

#include <stdint.h>

#include <vector>

#include "../rt_denoise.h"
#include "../rt_temporal.h"

struct rt_camera;
struct rt_denoise_params;
struct rt_temporal_params;
struct rt_variance_params;

namespace rtdn {

// The levels over the prepared state a (b: the other buffer; both are overwritten) and guides g (8 floats per pixel) of a W x rows
// picture; the last level's state goes out as out_rgb (3 floats per pixel) and out_var.
void RunLevelsHost(std::vector<rtd::DenoiseState>& a, std::vector<rtd::DenoiseState>& b, const std::vector<float>& g, uint32_t W, uint32_t rows,
                   const rtd::DenoiseParams& P, float* out_rgb, float* out_var);

// params (NULL: the defaults) into P; outside their domain: RT_ERR_INVALID_ARG with a message that starts with who.
int CheckDenoiseParams(const char* who, const rt_denoise_params* params, rtd::DenoiseParams* P);

// vparams (NULL: the moments source) into V; an unknown source, or a radius outside 1..3 under the spatial one: RT_ERR_INVALID_ARG with a
// message that starts with who.
int CheckVarianceParams(const char* who, const rt_variance_params* vparams, rtd::VarianceParams* V);

// The spatial prepare pass (../rt_denoise.h "the spatial variance source") over a W x rows strip: a[p] = (c0, v0), g = the guides (8 floats
// per pixel), both in image order; a and g are sized by the caller.  parts: NULL -- hdr and feat8 are the strip in image order -- or the
// layout of the gathered parts they are, read through the mapping (rt_denoise_launch.h).
struct ShardLayout;
void PrepareSpatialHost(const float* hdr, uint32_t n, const float* feat8, uint32_t m, uint32_t W, uint32_t rows, const ShardLayout* parts,
                        const rtd::DenoiseParams& P, uint32_t radius, std::vector<rtd::DenoiseState>& a, std::vector<float>& g);

// tparams (NULL: the defaults) into T; outside their domain: RT_ERR_INVALID_ARG with a message that starts with who.
int CheckTemporalParams(const char* who, const rt_temporal_params* tparams, rtd::TemporalParams* T);

// The same with the fetch chosen: a fetch that is neither RT_TEMPORAL_FETCH_NEAREST nor _BILINEAR is RT_ERR_INVALID_ARG, and NULL takes
// that fetch's defaults (rt_temporal_default_params_fetch).
int CheckTemporalParamsFetch(const char* who, const rt_temporal_params* tparams, uint32_t fetch, rtd::TemporalParams* T);

// The part of a camera record the reprojection reads.
rtd::TemporalCam CamOf(const rt_camera& c);

}  // namespace rtdn
