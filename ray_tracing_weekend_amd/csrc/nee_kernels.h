// nee_kernels.h -- host-visible description of the two queries an outside
// integrator needs next to the light pdf (rtw_occluded_rays / rtw_light_sample):
// their parameter block, the kernels that exist and the launch entry points of
// nee_f32.hip / nee_f64.hip.  They run on the plan of the other ray queries
// (host/query_plan.hpp: world, test form, stacks, LDS, light path) and on the
// queries' counters (query_kernels.h); nothing of the render's is touched.
#pragma once

#include "query_kernels.h"

namespace rtw {

// rtw_query_stats.is_light_pdf of the two queries
enum : uint32_t { kQueryAnyHit = 2, kQueryLightSample = 3 };

template <typename R>
struct NParams {
    DevScene<R> sc;
    // occlusion_kernel
    const R* rays;                    // n x 6 {o, d}
    const R* tmax;                    // n upper range ends, or null: +inf
    uint8_t* occluded;                // n x {0, 1}
    // light_sample_kernel
    const R* origins;                 // n x 3
    R* dirs;                          // n x 3
    R* pdf;                           // n, or null
    int32_t* light;                   // n list indices, or null
    uint64_t seed, first_stream;      // point k draws from Rng(seed, first_stream + k, sample)
    uint32_t sample;
    unsigned long long* counters;     // kQueryCounters (query_kernels.h)
    uint64_t n;
    R tmin;
    uint32_t stack;                   // per-lane traversal stack entries (BVH worlds, the light BVH)
};

// The kernels the library holds: those of the closest-hit query and of the light
// pdf (the same worlds, light paths and test forms).
constexpr bool occlusion_kernel_exists(bool f64, int world, bool robust) { return hit_kernel_exists(f64, world, robust); }
constexpr bool light_sample_kernel_exists(bool f64, int path, bool robust) {
    return light_kernel_exists(f64, path, robust);
}

// Launches (nee_f32.hip / nee_f64.hip) on `stream`: p.n > 0.  Each returns the
// world / light path launched, or -1 (no such kernel, or the launch failed).
// lds_bytes: QueryPlan::hit_lds / light_lds -- the any-hit stages what the
// closest-hit query stages; it leaves the stealing area unused.
int launch_occlusion(const NParams<float>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                     hipStream_t stream);
int launch_occlusion(const NParams<double>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                     hipStream_t stream);
int launch_light_sample(const NParams<float>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap,
                        hipStream_t stream);
int launch_light_sample(const NParams<double>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap,
                        hipStream_t stream);

}  // namespace rtw
