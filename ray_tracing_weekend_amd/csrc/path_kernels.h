// path_kernels.h -- host-visible description of the two path queries
// (rtw_camera_rays / rtw_shade_rays): their parameter blocks, the kernels that
// exist and the launch entry points of path_f32.hip / path_f64.hip.  The bounce
// runs on the light path of the other ray queries' plan (host/query_plan.hpp:
// light_path, light_stack, light_lds, robust) and on the queries' counters
// (query_kernels.h); nothing of the render's is touched.
#pragma once

#include "query_kernels.h"

namespace rtw {

// rtw_query_stats.is_light_pdf of the two queries
enum : uint32_t { kQueryCameraRays = 4, kQueryShade = 5 };
// SParams::event (RTW_EVENT_* of include/rtw.h)
enum : int32_t { kEventMiss = 0, kEventAbsorbed = 1, kEventReflect = 2, kEventScatter = 3 };

// camera_rays_kernel: the camera as a render's kernel sees it (host/camera_params.hpp
// fill_camera), the stream key and the rays asked for
template <typename R>
struct CParams {
    R center[3], p00[3], du[3], dv[3], disk_u[3], disk_v[3], bg[3];
    R u_scale;
    uint32_t defocus;
    uint32_t W;
    uint32_t sample;
    uint64_t seed;
    uint64_t n_pixels;                // W * H > 0: an index is clamped to n_pixels - 1
    const uint32_t* pixels;           // n pixel indices j * W + i, or null: first_pixel + k
    uint64_t first_pixel;
    uint64_t n;
    R* rays;                          // n x 6 {o, d}
    uint64_t* rng;                    // n x 4: s0..s3 after get_ray's draws
    unsigned long long* counters;     // kQueryCounters (query_kernels.h)
};

// shade_rays_kernel
template <typename R>
struct SParams {
    DevScene<R> sc;
    const R* rays;                    // n x 6 {o, d}: the incoming rays
    const R* hits;                    // n x 9, ids n x 4: hit_rays_kernel's records of them
    const int32_t* ids;
    uint64_t* rng;                    // n x 4, read and written back
    R* next;                          // n x 6 {p, direction}
    R* weight;                        // n x 3
    R* emitted;                       // n x 3
    int32_t* event;                   // n
    R* pdfs;                          // n x 3 {mixture, light list, scattering}, or null
    unsigned long long* counters;     // kQueryCounters
    uint64_t n;
    uint32_t stack;                   // the light BVH's per-lane stack entries
};

// The kernels the library holds: one camera kernel per precision; the bounce on
// every light path, in the test forms of the light pdf.
constexpr bool camera_rays_kernel_exists(bool) { return true; }
constexpr bool shade_rays_kernel_exists(bool f64, int path, bool robust) { return light_kernel_exists(f64, path, robust); }

// The widest aligned access a record of `bytes` allows, and the alignment its array
// must start on (checked by capi_path.cpp): the largest power of two dividing the
// stride, at most 16.
constexpr uint32_t record_align(size_t bytes) { return bytes % 16 == 0 ? 16u : bytes % 8 == 0 ? 8u : 4u; }

// Launches (path_f32.hip / path_f64.hip) on `stream`: p.n > 0.  launch_shade_rays
// returns the light path launched, launch_camera_rays 0; -1: no such kernel, or
// the launch failed.  lds_bytes: kQueryLdsMin / QueryPlan::light_lds.
int launch_camera_rays(const CParams<float>& p, size_t lds_bytes, uint32_t grid_cap,
                       hipStream_t stream);
int launch_camera_rays(const CParams<double>& p, size_t lds_bytes, uint32_t grid_cap,
                       hipStream_t stream);
int launch_shade_rays(const SParams<float>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap,
                      hipStream_t stream);
int launch_shade_rays(const SParams<double>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap,
                      hipStream_t stream);

}  // namespace rtw
