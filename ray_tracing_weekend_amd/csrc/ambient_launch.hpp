// ambient_launch.hpp -- host side of ambient_kernel: the kernel table of a unit,
// launched as the query kernels are (query_launch.hpp launch_table /
// launch_resident), one workgroup of work per 256 (point, sample) pairs.
// Included by ambient_f32.hip / ambient_f64.hip, which instantiate the kernels
// through it.
#pragma once

#include "ambient_kernel.hpp"
#include "query_launch.hpp"

namespace rtw {

template <typename R>
struct AmbientEntry {
    template <int kWorld, bool kRobust>
    static int run(const AParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (ambient_kernel_exists(sizeof(R) == 8, kWorld, kRobust))
            return launch_resident(&dev::ambient_kernel<R, kWorld, kRobust>,
                                   (p.n * p.n_samples + kQueryBlock - 1) / kQueryBlock, p, lds_bytes, grid_cap,
                                   stream) ? -1 : kWorld;
        else
            return -1;
    }
};

// (defined by the unit of each precision)
#define RTW_AMBIENT_UNIT(R)                                                                             \
    int launch_ambient(const AParams<R>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap, \
                       hipStream_t stream) {                                                            \
        return launch_table<AmbientEntry<R>>(p, world, robust, lds_bytes, grid_cap, stream,             \
                                             std::make_index_sequence<2 * (kWorldBvhLds + 1)>());       \
    }

}  // namespace rtw
