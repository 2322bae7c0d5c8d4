// path_launch.hpp -- host side of camera_rays_kernel / shade_rays_kernel: the
// kernel table of a unit, launched as the query kernels are (query_launch.hpp
// launch_table / launch_resident).  Included by path_f32.hip / path_f64.hip, which
// instantiate the kernels through it.
#pragma once

#include "path_kernel.hpp"
#include "query_launch.hpp"

namespace rtw {

template <typename R>
struct ShadeEntry {
    template <int kPath, bool kRobust>
    static int run(const SParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (shade_rays_kernel_exists(sizeof(R) == 8, kPath, kRobust))
            return launch_resident(&dev::shade_rays_kernel<R, kPath, kRobust>, (p.n + kQueryBlock - 1) / kQueryBlock,
                                   p, lds_bytes, grid_cap, stream) ? -1 : kPath;
        else
            return -1;
    }
};

// (defined by the unit of each precision)
#define RTW_PATH_UNIT(R)                                                                                   \
    int launch_camera_rays(const CParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) { \
        return launch_resident(&dev::camera_rays_kernel<R>, (p.n + kQueryBlock - 1) / kQueryBlock, p,      \
                               lds_bytes, grid_cap, stream);                                               \
    }                                                                                                      \
    int launch_shade_rays(const SParams<R>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap, \
                          hipStream_t stream) {                                                            \
        return launch_table<ShadeEntry<R>>(p, path, robust, lds_bytes, grid_cap, stream,                   \
                                           std::make_index_sequence<2 * kLightPaths>());                   \
    }

}  // namespace rtw
