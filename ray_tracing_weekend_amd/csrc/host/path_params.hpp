// path_params.hpp -- the kernel parameters of the two path queries
// (rtw_camera_rays / rtw_shade_rays), built from the camera and from the plan of
// the other ray queries (query_plan.hpp).  The buffers and the counters are the
// caller's: null here.  Host only, no HIP call, so that the CPU can check them
// (tests/native/path_plan_check.cpp).
#pragma once

#include "../path_kernels.h"
#include "camera_params.hpp"
#include "query_plan.hpp"

namespace rtw {

// The camera as a render's kernel sees it (fill_camera) and the stream key: ray k
// is pixel pixels[k] / first_pixel + k of sample `sample`.
template <typename R>
inline CParams<R> camera_ray_params(const rtw_camera& cam, uint64_t seed, uint32_t sample, uint64_t first_pixel,
                                    uint64_t n) {
    CParams<R> p{};
    fill_camera<R>(p, cam);
    p.W = cam.image_width;
    p.n_pixels = (uint64_t)cam.image_width * cam.image_height;
    p.seed = seed;
    p.sample = sample;
    p.first_pixel = first_pixel;
    p.n = n;
    return p;
}

// The bounce on the plan's light path, with its test form and the light BVH's stack.
template <typename R>
inline SParams<R> shade_params(const DevScene<R>& sc, const QueryPlan& q, uint64_t n) {
    SParams<R> p{};
    p.sc = sc;
    p.sc.robust = q.robust;
    p.stack = q.light_stack;
    p.n = n;
    return p;
}

// What a bounce launch asks for: the kernel <path, robust> and its dynamic LDS
struct ShadeLaunch {
    int path;
    bool robust;
    size_t lds;
};
inline ShadeLaunch shade_launch(const QueryPlan& q) { return ShadeLaunch{q.light_path, q.robust != 0, q.light_lds}; }

}  // namespace rtw
