// features_launch.hpp -- host side of the feature kernels: the table of the
// kernels a unit holds (the world and the test form are host/query_plan.cpp's
// decision; hit_kernel_exists names the entries) and their grid.  Included by
// features_f32.hip / features_f64.hip, which instantiate the kernels through it.
#pragma once

#include <algorithm>
#include <utility>

#include "features_kernel.hpp"

namespace rtw {

// Grid of a feature pass: one wave per tile, no more workgroups than fit on the
// GPU at once for this kernel and LDS size -- the waves take their tiles from a
// counter, so what a workgroup stages into LDS is paid once.
template <typename K>
inline uint32_t features_grid(K kernel, uint32_t n_tiles, size_t lds_bytes) {
    const uint64_t blocks = ((uint64_t)n_tiles + kQueryWaves - 1) / kQueryWaves;
    int per_cu = 0, dev = 0, cus = 0;
    uint64_t resident = 2048;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), (int)kQueryBlock,
                                                     lds_bytes) == hipSuccess &&
        hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per_cu >= 1 && cus >= 1)
        resident = (uint64_t)per_cu * cus;
    return (uint32_t)std::min<uint64_t>(blocks, resident);
}

template <typename R, typename K>
inline int features_launch(K kernel, const FParams<R>& p, size_t lds_bytes, hipStream_t stream) {
    // dynamic LDS above 64 KiB must be allowed per kernel
    if (lds_bytes > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes);
    hipLaunchKernelGGL(kernel, dim3(features_grid(kernel, p.n_tiles, lds_bytes)), dim3(kQueryBlock), lds_bytes, stream,
                       p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// entry I of the table: <world I / 2, robust I % 2>
template <typename R, int kWorld, bool kRobust>
inline int features_entry(const FParams<R>& p, size_t lds_bytes, hipStream_t stream) {
    if constexpr (hit_kernel_exists(sizeof(R) == 8, kWorld, kRobust))
        return features_launch(&dev::primary_features_kernel<R, kWorld, kRobust>, p, lds_bytes, stream) ? -1 : kWorld;
    else
        return -1;
}
template <typename R, size_t... I>
inline int launch_features_impl(const FParams<R>& p, int world, bool robust, size_t lds_bytes, hipStream_t stream,
                                std::index_sequence<I...>) {
    int ran = -1;   // (no such entry)
    (void)((world == (int)I / 2 && robust == (I % 2 != 0) &&
            ((ran = features_entry<R, (int)I / 2, I % 2 != 0>(p, lds_bytes, stream)), true)) || ...);
    return ran;
}

// (defined by the unit of each precision)
#define RTW_FEATURES_UNIT(R)                                                                                          \
    int launch_primary_features(const FParams<R>& p, int world, bool robust, size_t lds_bytes, hipStream_t stream) { \
        return launch_features_impl<R>(p, world, robust, lds_bytes, stream,                                          \
                                       std::make_index_sequence<2 * (kWorldBvhLds + 1)>());                          \
    }

}  // namespace rtw
