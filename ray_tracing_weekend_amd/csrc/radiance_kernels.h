// radiance_kernels.h -- host-visible description of the radiance query
// (rtw_radiance_rays): its parameter block, the kernels that exist, its dynamic
// LDS and the launch entry points of radiance_f32.hip / radiance_f64.hip.  It
// runs on the plan of the other ray queries (host/query_plan.hpp: world, test
// form, stacks, LDS, light path) and on the queries' counters (query_kernels.h);
// nothing of the render's or of the other queries' is touched.
#pragma once

#include "direct_kernels.h"

namespace rtw {

// rtw_query_stats.is_light_pdf of the query
enum : uint32_t { kQueryRadiance = 10 };

template <typename R>
struct RParams {
    DevScene<R> sc;
    const R* rays;                    // n x 6 {origin, direction}
    double* radiance;                 // n x 3 f64 sums
    R* colours;                       // n * n_samples x 3, or null
    uint32_t* segments;               // n * n_samples, or null
    uint64_t* rng;                    // n x 4 start states, read and written back, or null: seeded
    uint64_t seed, first_stream;      // ray k, sample s draws from Rng(seed, first_stream + k, s)
    uint32_t first_sample, n_samples;
    uint32_t max_depth;
    uint32_t accumulate;              // continue `radiance` from its content
    int32_t light_path;               // LightPath of the plan: a wave-uniform switch in the kernel
    unsigned long long* counters;     // kQueryCounters (query_kernels.h)
    uint64_t n;
    R tmin;                           // f64::EPSILON in the context's precision
    R bg[3];                          // the background
    uint32_t stack;                   // per-lane traversal stack entries (BVH worlds)
    uint32_t light_stack;             // ... of the light BVH
    uint32_t light_off;               // byte offset of the light BVH's stacks in the dynamic LDS
};

// Dynamic LDS of radiance_kernel<R, world>: direct_light_kernel's layout
// (direct_kernels.h direct_lds): the closest-hit query's bytes at its offsets,
// then -- the light BVH only -- that walk's per-lane stacks.
inline size_t radiance_lds(size_t hit_lds, int light_path, uint32_t light_stack) {
    return direct_lds(hit_lds, light_path, light_stack);
}

// The trips a lane's loop may take: S paths of at most max(max_depth, 1) segments
// each (a path of depth 0 takes one trip to fold its black colour).
constexpr uint64_t radiance_trip_bound(uint32_t n_samples, uint32_t max_depth) {
    return (uint64_t)n_samples * (uint64_t)(max_depth ? max_depth : 1u);
}

// The kernels the library holds: one per closest-hit kernel; the light path is no
// template axis.
constexpr bool radiance_kernel_exists(bool f64, int world, bool robust) { return hit_kernel_exists(f64, world, robust); }

// Launches (radiance_f32.hip / radiance_f64.hip) on `stream`: p.n > 0.  Each
// returns the world launched, or -1 (no such kernel, or the launch failed).
int launch_radiance(const RParams<float>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                    hipStream_t stream);
int launch_radiance(const RParams<double>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                    hipStream_t stream);

}  // namespace rtw
