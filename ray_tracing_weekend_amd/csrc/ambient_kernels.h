// ambient_kernels.h -- host-visible description of the ambient-occlusion query
// (rtw_ambient_occlusion): its parameter block, the kernels that exist and the
// launch entry points of ambient_f32.hip / ambient_f64.hip.  It runs on the plan
// of the other ray queries (host/query_plan.hpp: world, test form, stack, the
// closest hit's LDS unchanged) and on the queries' counters (query_kernels.h);
// nothing of the render's or of the other queries' is touched.
#pragma once

#include "nee_kernels.h"

namespace rtw {

// rtw_query_stats.is_light_pdf of the query
enum : uint32_t { kQueryAmbient = 9 };

template <typename R>
struct AParams {
    DevScene<R> sc;
    const R* points;                  // n x 6 {p, normal}
    uint32_t* open;                   // n counts: zeroed or continued by the host, added to here
    R* directions;                    // n * n_samples x 3, or null
    uint8_t* occluded;                // n * n_samples x {0, 1}, or null
    uint64_t seed, first_stream;      // point k, sample s draws from Rng(seed, first_stream + k, s)
    uint32_t first_sample, n_samples;
    unsigned long long* counters;     // kQueryCounters (query_kernels.h)
    uint64_t n;
    R tmin, tmax;                     // the range of every pair's any hit
    uint32_t stack;                   // per-lane traversal stack entries (BVH worlds)
};

// The kernels the library holds: one per any-hit kernel (the same worlds and test forms).
constexpr bool ambient_kernel_exists(bool f64, int world, bool robust) {
    return occlusion_kernel_exists(f64, world, robust);
}

// Launches (ambient_f32.hip / ambient_f64.hip) on `stream`: p.n * p.n_samples > 0.
// Each returns the world launched, or -1 (no such kernel, or the launch failed).
// lds_bytes: QueryPlan::hit_lds, as the any-hit query's.
int launch_ambient(const AParams<float>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                   hipStream_t stream);
int launch_ambient(const AParams<double>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                   hipStream_t stream);

}  // namespace rtw
