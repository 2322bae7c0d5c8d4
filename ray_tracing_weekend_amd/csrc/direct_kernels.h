// direct_kernels.h -- host-visible description of the direct-lighting query
// (rtw_direct_light): its parameter block, the kernels that exist, its dynamic
// LDS and the launch entry points of direct_f32.hip / direct_f64.hip.  It runs
// on the plan of the other ray queries (host/query_plan.hpp: world, test form,
// stacks, LDS, light path) and on the queries' counters (query_kernels.h);
// nothing of the render's or of the other queries' is touched.
#pragma once

#include "query_kernels.h"

namespace rtw {

// rtw_query_stats.is_light_pdf of the query
enum : uint32_t { kQueryDirectLight = 8 };

// values per row of the optional records: {d xyz, pdf, t, spdf, Le rgb, term rgb} and
// {light-list index, object id or -1, material id, 1 if the sample added a term}
constexpr uint32_t kDirectSampleValues = 12, kDirectIdValues = 4;

template <typename R>
struct DParams {
    DevScene<R> sc;
    const R* points;                  // n x 6 {p, normal}
    double* direct;                   // n x 3 f64 sums
    R* samples;                       // n * n_samples x 12, or null
    int32_t* sample_ids;              // n * n_samples x 4, or null
    uint64_t seed, first_stream;      // point k, sample s draws from Rng(seed, first_stream + k, s)
    uint32_t first_sample, n_samples;
    uint32_t accumulate;              // continue `direct` from its content
    int32_t light_path;               // LightPath of the plan: a wave-uniform switch in the kernel
    unsigned long long* counters;     // kQueryCounters (query_kernels.h)
    uint64_t n;
    R tmin;
    uint32_t stack;                   // per-lane traversal stack entries (BVH worlds)
    uint32_t light_stack;             // ... of the light BVH
    uint32_t light_off;               // byte offset of the light BVH's stacks in the dynamic LDS
};

// Dynamic LDS of direct_light_kernel<R, world>: the closest-hit query's bytes at
// its offsets (query_hit_lds), then -- the light BVH only -- that walk's per-lane
// stacks (query_light_lds), from the next 16-byte boundary.
inline size_t direct_light_off(size_t hit_lds) { return (hit_lds + 15u) & ~(size_t)15u; }
inline size_t direct_lds(size_t hit_lds, int light_path, uint32_t light_stack) {
    return light_path == kLightBvh ? direct_light_off(hit_lds) + query_light_lds(kLightBvh, light_stack) : hit_lds;
}

// The kernels the library holds: one per closest-hit kernel; the light path is no
// template axis.
constexpr bool direct_kernel_exists(bool f64, int world, bool robust) { return hit_kernel_exists(f64, world, robust); }

// Launches (direct_f32.hip / direct_f64.hip) on `stream`: p.n > 0.  Each returns the
// world launched, or -1 (no such kernel, or the launch failed).
int launch_direct_light(const DParams<float>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                        hipStream_t stream);
int launch_direct_light(const DParams<double>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,
                        hipStream_t stream);

}  // namespace rtw
