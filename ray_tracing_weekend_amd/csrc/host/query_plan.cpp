// query_plan.cpp -- see query_plan.hpp
#include "query_plan.hpp"

#include <algorithm>

#include "camera_params.hpp"
#include "tiles.hpp"

namespace rtw {

template <typename R>
QueryPlan plan_query(const RenderKnobs& k, const DevScene<R>& sc, const SceneScale& scale, const double* center) {
    QueryPlan q;
    RenderPlan p;
    const double origin[3] = {0.0, 0.0, 0.0};
    plan_world<R>(k, sc, center ? center : origin, scale, p);
    q.accel = p.accel;
    q.world = p.world;
    q.robust = sizeof(R) == 4 ? p.robust : 0u;
    q.err = p.err;
    q.err_text = p.err_text;
    if (q.err) return q;
    // The traversal stack: what the tree needs (plan_world's also covers the render
    // kernel's light walks, which a hit query does not run).  The stack bounds were
    // checked by plan_world: bvh4_stack + 1, bvh_depth <= kBvhStack.
    if (q.world == kWorldBvh4) q.stack = sc.bvh4_stack + 1;
    else if (q.world >= kWorldBvh) q.stack = std::max(sc.bvh_depth, 1u);
    q.hit_lds = query_hit_lds<R>(q.world, q.stack, sc.n_nodes, sc.n_sph);
    // the tree in LDS: the query stages the head of the render kernel's layout, so
    // it fits whenever the render's does
    if (q.hit_lds > kLdsLimit) {
        q.err = RTW_E_UNSUPPORTED;
        q.err_text = "the query kernel's LDS exceeds the device's";
        return q;
    }
    // the light path, as render_kernel's Lambertian bounce picks it: the mixed list
    // when there is one, else the light grid / BVH of the plan, else the linear list
    q.light_path = sc.lref ? kLightMixed : (p.light_bvh == 2 ? kLightGrid : (p.light_bvh == 1 ? kLightBvh : kLightLinear));
    q.light_stack = q.light_path == kLightBvh ? sc.lbvh_depth + 1 : 1u;
    q.light_lds = query_light_lds(q.light_path, q.light_stack);
    if (!hit_kernel_exists(sizeof(R) == 8, q.world, q.robust != 0) ||
        !light_kernel_exists(sizeof(R) == 8, q.light_path, q.robust != 0)) {
        q.err = RTW_E_UNSUPPORTED;
        q.err_text = "no query kernel for this scene and tuning";
    }
    return q;
}

template <typename R>
FParams<R> feature_params(const DevScene<R>& sc, const rtw_camera& cam, uint64_t seed, uint32_t first, uint32_t n,
                          const QueryPlan& q) {
    FParams<R> p{};
    p.sc = sc;
    p.sc.robust = q.robust;
    fill_camera<R>(p, cam);
    p.seed = seed;
    p.W = cam.image_width;
    p.H = cam.image_height;
    p.first = first;
    p.end = first + n;
    p.tiles_x = tiles_across(p.W);
    p.n_tiles = p.tiles_x * tiles_across(p.H);
    p.stack = q.stack;
    return p;
}

template FParams<float> feature_params<float>(const DevScene<float>&, const rtw_camera&, uint64_t, uint32_t, uint32_t,
                                              const QueryPlan&);
template FParams<double> feature_params<double>(const DevScene<double>&, const rtw_camera&, uint64_t, uint32_t,
                                                uint32_t, const QueryPlan&);
template QueryPlan plan_query<float>(const RenderKnobs&, const DevScene<float>&, const SceneScale&, const double*);
template QueryPlan plan_query<double>(const RenderKnobs&, const DevScene<double>&, const SceneScale&, const double*);

}  // namespace rtw
