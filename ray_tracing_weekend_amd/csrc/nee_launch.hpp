// nee_launch.hpp -- host side of occlusion_kernel / light_sample_kernel: the
// kernel tables of a unit, launched as the query kernels are (query_launch.hpp
// launch_table / launch_resident).  Included by nee_f32.hip / nee_f64.hip, which
// instantiate the kernels through it.
#pragma once

#include "nee_kernel.hpp"
#include "query_launch.hpp"

namespace rtw {

template <typename R>
struct OcclusionEntry {
    template <int kWorld, bool kRobust>
    static int run(const NParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (occlusion_kernel_exists(sizeof(R) == 8, kWorld, kRobust))
            return launch_resident(&dev::occlusion_kernel<R, kWorld, kRobust>, (p.n + kQueryBlock - 1) / kQueryBlock, p,
                                   lds_bytes, grid_cap, stream) ? -1 : kWorld;
        else
            return -1;
    }
};
template <typename R>
struct LightSampleEntry {
    template <int kPath, bool kRobust>
    static int run(const NParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (light_sample_kernel_exists(sizeof(R) == 8, kPath, kRobust))
            return launch_resident(&dev::light_sample_kernel<R, kPath, kRobust>,
                                   (p.n + kQueryBlock - 1) / kQueryBlock, p, lds_bytes, grid_cap, stream) ? -1 : kPath;
        else
            return -1;
    }
};

// (defined by the unit of each precision)
#define RTW_NEE_UNIT(R)                                                                                      \
    int launch_occlusion(const NParams<R>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,   \
                         hipStream_t stream) {                                                               \
        return launch_table<OcclusionEntry<R>>(p, world, robust, lds_bytes, grid_cap, stream,                \
                                               std::make_index_sequence<2 * (kWorldBvhLds + 1)>());          \
    }                                                                                                        \
    int launch_light_sample(const NParams<R>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap, \
                            hipStream_t stream) {                                                            \
        return launch_table<LightSampleEntry<R>>(p, path, robust, lds_bytes, grid_cap, stream,               \
                                                 std::make_index_sequence<2 * kLightPaths>());               \
    }

}  // namespace rtw
