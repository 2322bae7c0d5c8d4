// radiance_launch.hpp -- host side of radiance_kernel: the kernel table of a
// unit, launched as the query kernels are (query_launch.hpp launch_table /
// launch_resident).  Included by radiance_f32.hip / radiance_f64.hip, which
// instantiate the kernels through it.
#pragma once

#include "query_launch.hpp"
#include "radiance_kernel.hpp"

namespace rtw {

template <typename R>
struct RadianceEntry {
    template <int kWorld, bool kRobust>
    static int run(const RParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (radiance_kernel_exists(sizeof(R) == 8, kWorld, kRobust))
            return launch_resident(&dev::radiance_kernel<R, kWorld, kRobust>,
                                   (p.n + kQueryBlock - 1) / kQueryBlock, p, lds_bytes, grid_cap, stream) ? -1 : kWorld;
        else
            return -1;
    }
};

// (defined by the unit of each precision)
#define RTW_RADIANCE_UNIT(R)                                                                              \
    int launch_radiance(const RParams<R>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap, \
                        hipStream_t stream) {                                                             \
        return launch_table<RadianceEntry<R>>(p, world, robust, lds_bytes, grid_cap, stream,              \
                                              std::make_index_sequence<2 * (kWorldBvhLds + 1)>());        \
    }

}  // namespace rtw
