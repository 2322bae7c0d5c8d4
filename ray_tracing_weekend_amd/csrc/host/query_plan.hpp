// query_plan.hpp -- what a batched ray query launches (rtw_hit_rays /
// rtw_light_pdf_rays): the world, the test form, the traversal stack and the
// dynamic LDS of hit_rays_kernel, and the light path of light_pdf_rays_kernel.
// A query runs the traversal a render of the scene would run under the same
// tuning keys: the world and the light path are render_plan.hpp plan_world's.
// The feature pass (rtw_render_features) runs on the same plan: its kernel
// parameters are feature_params'.  Host only, no HIP call.
#pragma once

#include "../features_kernels.h"   // FParams, for feature_params (it includes query_kernels.h)
#include "render_plan.hpp"

namespace rtw {

struct QueryPlan {
    int accel = RTW_ACCEL_BRUTE;        // RTW_ACCEL_AUTO resolved
    int world = kWorldLds;              // WorldMode of hit_rays_kernel
    uint32_t robust = 0;                // f32: the closest-approach sphere / light tests
    uint32_t stack = 1;                 // traversal stack entries per lane (BVH worlds)
    size_t hit_lds = kQueryLdsMin;      // dynamic LDS of hit_rays_kernel
    int light_path = kLightLinear;      // LightPath of light_pdf_rays_kernel
    uint32_t light_stack = 1;           // the light BVH's stack entries per lane
    size_t light_lds = kQueryLdsMin;    // dynamic LDS of light_pdf_rays_kernel
    int err = RTW_OK;
    const char* err_text = "";
};

// A query has no camera: knob robust = 2 judges the scene's scale from the origin
// (center null).  The feature pass (rtw_render_features) traces a camera's primary
// rays with the query's plan: it passes the camera's center, as a render plan does.
template <typename R>
QueryPlan plan_query(const RenderKnobs& k, const DevScene<R>& sc, const SceneScale& scale,
                     const double* center = nullptr);

// The grid of a query, feature or wavefront launch (query_launch.hpp launch_resident):
// `blocks` workgroups of work, no more than `resident` fit on the GPU at once, and
// no more than tuning "query_grid" allows (cap 0: no cap).  Never 0 for blocks > 0:
// a workgroup walks its blocks grid-stride (or takes tiles from a counter), so one
// workgroup does all the work of any launch.
inline uint32_t query_grid(uint64_t blocks, uint64_t resident, uint32_t cap) {
    uint64_t g = blocks < resident ? blocks : resident;
    if (cap && cap < g) g = cap;
    if (g == 0 && blocks) g = 1;
    return (uint32_t)(g < 0xFFFFFFFFull ? g : 0xFFFFFFFFull);
}

// The kernel parameters of a feature pass planned as `q` (with the camera's
// center): the scene, the camera as a render's kernel sees it (camera_params.hpp),
// the samples [first, first + n) and the image's tiles.  The buffers (counts,
// features, ids) and the counters are the caller's: null here.
template <typename R>
FParams<R> feature_params(const DevScene<R>& sc, const rtw_camera& cam, uint64_t seed, uint32_t first, uint32_t n,
                          const QueryPlan& q);

}  // namespace rtw
