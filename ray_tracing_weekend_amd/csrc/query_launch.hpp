// query_launch.hpp -- host side of the query kernels: a table of the kernels
// a unit holds (the world / light path and the test form are host/query_plan.cpp's
// decision) and their grids.  Included by query_f32.hip / query_f64.hip, which
// instantiate the kernels through it.
#pragma once

#include <algorithm>
#include <utility>

#include "query_kernel.hpp"

namespace rtw {

// Grid of a query: one workgroup per 256 rays, no more than fit on the GPU at
// once for this kernel and LDS size -- a workgroup loops over ray blocks, so
// what it stages into LDS is paid once.
template <typename K>
inline uint32_t query_grid(K kernel, uint64_t n, size_t lds_bytes) {
    const uint64_t blocks = (n + kQueryBlock - 1) / kQueryBlock;
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
inline int query_launch(K kernel, const QParams<R>& p, size_t lds_bytes, hipStream_t stream) {
    // dynamic LDS above 64 KiB must be allowed per kernel
    if (lds_bytes > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes);
    hipLaunchKernelGGL(kernel, dim3(query_grid(kernel, p.n, lds_bytes)), dim3(kQueryBlock), lds_bytes, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// entry I of the hit table: <world I / 2, robust I % 2>; of the light table: <path I / 2, robust I % 2>
template <typename R, int kWorld, bool kRobust>
inline int hit_entry(const QParams<R>& p, size_t lds_bytes, hipStream_t stream) {
    if constexpr (hit_kernel_exists(sizeof(R) == 8, kWorld, kRobust))
        return query_launch(&dev::hit_rays_kernel<R, kWorld, kRobust>, p, lds_bytes, stream) ? -1 : kWorld;
    else
        return -1;
}
template <typename R, int kPath, bool kRobust>
inline int light_entry(const QParams<R>& p, size_t lds_bytes, hipStream_t stream) {
    if constexpr (light_kernel_exists(sizeof(R) == 8, kPath, kRobust))
        return query_launch(&dev::light_pdf_rays_kernel<R, kPath, kRobust>, p, lds_bytes, stream) ? -1 : kPath;
    else
        return -1;
}
template <typename R, size_t... I>
inline int launch_hit_impl(const QParams<R>& p, int world, bool robust, size_t lds_bytes, hipStream_t stream,
                           std::index_sequence<I...>) {
    int ran = -1;   // (no such entry)
    (void)((world == (int)I / 2 && robust == (I % 2 != 0) &&
            ((ran = hit_entry<R, (int)I / 2, I % 2 != 0>(p, lds_bytes, stream)), true)) || ...);
    return ran;
}
template <typename R, size_t... I>
inline int launch_light_impl(const QParams<R>& p, int path, bool robust, size_t lds_bytes, hipStream_t stream,
                             std::index_sequence<I...>) {
    int ran = -1;
    (void)((path == (int)I / 2 && robust == (I % 2 != 0) &&
            ((ran = light_entry<R, (int)I / 2, I % 2 != 0>(p, lds_bytes, stream)), true)) || ...);
    return ran;
}

// (defined by the unit of each precision)
#define RTW_QUERY_UNIT(R)                                                                                         \
    int launch_hit_rays(const QParams<R>& p, int world, bool robust, size_t lds_bytes, hipStream_t stream) {      \
        return launch_hit_impl<R>(p, world, robust, lds_bytes, stream,                                            \
                                  std::make_index_sequence<2 * (kWorldBvhLds + 1)>());                            \
    }                                                                                                             \
    int launch_light_pdf_rays(const QParams<R>& p, int path, bool robust, size_t lds_bytes, hipStream_t stream) { \
        return launch_light_impl<R>(p, path, robust, lds_bytes, stream, std::make_index_sequence<2 * kLightPaths>()); \
    }

}  // namespace rtw
