// stage_scene.hpp -- the caller's f64 scene (include/rtw.h rtw_scene) checked
// and converted into the device layout of rtw_kernels.h, in one host blob.
// Host only, no HIP call: the C-ABI uploads the blob.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../../include/rtw.h"
#include "../rtw_kernels.h"
#include "bvh.hpp"

namespace rtw {

// Quad::new (quadrilateral.rs:37-56) in f64: out = kQuadR values
void quad_derive(const double* p, double* out);
// Transformed<Cuboid> derived record in f64: out = kBoxR values
void box_derive(const double* b, double* out);

// Convert the caller's f64 SoA into the device layout of precision R, in one
// host staging blob, and fill the DevScene pointers relative to `base`.
// keep_bvh (may be null) receives the binary BVH over the spheres that was
// staged (the tile classifier walks it on the host, host/tile_cull.hpp).
template <typename R>
std::vector<unsigned char> stage_scene(const rtw_scene* s, DevScene<R>* ds, uintptr_t base, uint32_t leaf_max,
                                       uint32_t light_leaf, double grid_density, BvhBuild* keep_bvh = nullptr);
extern template std::vector<unsigned char> stage_scene<float>(const rtw_scene*, DevScene<float>*, uintptr_t,
                                                              uint32_t, uint32_t, double, BvhBuild*);
extern template std::vector<unsigned char> stage_scene<double>(const rtw_scene*, DevScene<double>*, uintptr_t,
                                                               uint32_t, uint32_t, double, BvhBuild*);

// RTW_OK, or the error code with its text in *msg
int validate_scene(const rtw_scene* s, std::string* msg);

// Scale of a staged scene: for the f32 test choice (knob robust = 2) and the
// longest-tiles-first heuristic (render_plan.hpp plan_render)
struct SceneScale {
    double extent = 0.0, min_radius = 0.0;   // largest |coordinate| + radius; smallest radius > 0 (inf: none)
    size_t tree_bytes = 0;                   // the BVH nodes + leaf spheres + ids
};
template <typename R>
SceneScale scene_scale(const rtw_scene* s, const DevScene<R>& ds);

// spheres per BVH leaf of a scene of n_spheres (knob bvh_leaf, 0 = auto)
uint32_t auto_leaf(uint32_t bvh_leaf, uint32_t n_spheres, bool f64);

}  // namespace rtw
