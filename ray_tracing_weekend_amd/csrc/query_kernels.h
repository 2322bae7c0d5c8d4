// query_kernels.h -- host-visible description of the batched ray queries
// (rtw_hit_rays / rtw_light_pdf_rays): their parameter block, the kernels that
// exist and the launch entry points of query_f32.hip / query_f64.hip.  The
// queries read the staged scene (rtw_kernels.h DevScene) and nothing of the
// render's: their own parameters, counters and kernels.
#pragma once

#include "rtw_kernels.h"

namespace rtw {

constexpr uint32_t kQueryWaves = 4;              // 256-thread workgroups, one ray per lane
constexpr uint32_t kQueryBlock = 64 * kQueryWaves;
// the light path of light_pdf_rays_kernel (as the render selects it: RenderPlan::light_bvh,
// or the mixed list when DevScene::lref is set)
enum LightPath : int { kLightLinear = 0, kLightBvh = 1, kLightGrid = 2, kLightMixed = 3 };
constexpr int kLightPaths = 4;
// QParams::counters
enum : int { kQcRays = 0, kQcHits, kQcNodeVisits, kQcSphereTests, kQcLightTests, kQueryCounters };
// primitive kinds of a hit (RTW_PRIM_* of include/rtw.h)
enum : int32_t { kPrimPlane = 0, kPrimQuad = 1, kPrimCuboid = 2, kPrimSphere = 3 };

template <typename R>
struct QParams {
    DevScene<R> sc;
    const R* rays;                    // n x 6 {o, d}
    R* hits;                          // n x 9 {t, p, normal, u, v}     (hit_rays_kernel)
    int32_t* ids;                     // n x 4 {object, material, front, kind}
    R* pdf;                           // n                              (light_pdf_rays_kernel)
    unsigned long long* counters;     // kQueryCounters
    uint64_t n;
    R tmin;
    uint32_t stack;                   // per-lane traversal stack entries (BVH worlds, the light BVH)
};

// Dynamic LDS of hit_rays_kernel<R, world>.  Every launch holds at least
// kQueryLdsMin bytes: the workgroup's counters are summed there at the end.
//   kWorldLds:    the sphere list {c, r^2}
//   kWorldBvh..4: the traversal stacks + stealing area (traversal_lds)
//   kWorldBvhLds: traversal_lds | f32 nodes | f32 leaf spheres | ids (padded to 8) --
//                 the head of the render kernel's layout (render_kernel.hpp), so never
//                 more than the render plan allowed for the same tree
constexpr size_t kQueryLdsMin = 64;
template <typename R>
__host__ __device__ inline size_t query_hit_lds(int world, uint32_t stack, uint32_t n_nodes, uint32_t n_sph) {
    size_t b = 0;
    if (world == kWorldLds) b = (size_t)n_sph * sizeof(R4<R>);
    else if (world >= kWorldBvh) b = traversal_lds<R>(stack, false, kQueryWaves);
    if (world == kWorldBvhLds)
        b += (size_t)n_nodes * sizeof(BvhNode<float>) + (size_t)n_sph * sizeof(R4<float>) +
             (size_t)((n_sph + 7u) & ~7u) * sizeof(uint32_t);
    return b < kQueryLdsMin ? kQueryLdsMin : b;
}
// ... of light_pdf_rays_kernel: the light BVH's per-lane stacks
__host__ __device__ inline size_t query_light_lds(int path, uint32_t stack) {
    const size_t b = path == kLightBvh ? (size_t)kQueryBlock * stack * sizeof(int32_t) : 0;
    return b < kQueryLdsMin ? kQueryLdsMin : b;
}

// The kernels the library holds: every world, every light path; the
// closest-approach tests (robust) are f32's.
constexpr bool hit_kernel_exists(bool f64, int world, bool robust) {
    return world >= kWorldGlobal && world <= kWorldBvhLds && !(f64 && robust);
}
constexpr bool light_kernel_exists(bool f64, int path, bool robust) {
    return path >= 0 && path < kLightPaths && !(f64 && robust);
}

// Launches (query_f32.hip / query_f64.hip) on `stream`: p.n > 0.  Each returns
// the world / light path launched, or -1 (no such kernel, or the launch failed).
// grid_cap: tuning "query_grid" -- at most that many workgroups (0: the resident grid),
// for these and every other launch of query_launch.hpp's launch_resident.
int launch_hit_rays(const QParams<float>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                    hipStream_t stream);
int launch_hit_rays(const QParams<double>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                    hipStream_t stream);
int launch_light_pdf_rays(const QParams<float>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap,
                          hipStream_t stream);
int launch_light_pdf_rays(const QParams<double>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap,
                          hipStream_t stream);

}  // namespace rtw
