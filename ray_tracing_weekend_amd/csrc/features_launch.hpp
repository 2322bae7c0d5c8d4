// features_launch.hpp -- host side of the feature kernels: the table of the
// kernels a unit holds (the world and the test form are host/query_plan.cpp's
// decision; hit_kernel_exists names the entries) and their grid.  Included by
// features_f32.hip / features_f64.hip, which instantiate the kernels through it.
#pragma once

#include "features_kernel.hpp"
#include "query_launch.hpp"

namespace rtw {

// one wave per tile, on the resident grid of query_launch.hpp
template <typename R>
struct FeaturesEntry {
    template <int kWorld, bool kRobust>
    static int run(const FParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (hit_kernel_exists(sizeof(R) == 8, kWorld, kRobust)) {
            const uint64_t blocks = ((uint64_t)p.n_tiles + kQueryWaves - 1) / kQueryWaves;
            return launch_resident(&dev::primary_features_kernel<R, kWorld, kRobust>, blocks, p, lds_bytes, grid_cap,
                                   stream) ? -1 : kWorld;
        } else {
            return -1;
        }
    }
};

// (defined by the unit of each precision)
#define RTW_FEATURES_UNIT(R)                                                                                      \
    int launch_primary_features(const FParams<R>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap, \
                                hipStream_t stream) {                                                             \
        return launch_table<FeaturesEntry<R>>(p, world, robust, lds_bytes, grid_cap, stream,                      \
                                              std::make_index_sequence<2 * (kWorldBvhLds + 1)>());                \
    }

}  // namespace rtw
