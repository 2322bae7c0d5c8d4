// query_launch.hpp -- host side of the query kernels: a table of the kernels
// a unit holds (the world / light path and the test form are host/query_plan.cpp's
// decision) and their grids.  Included by query_f32.hip / query_f64.hip, which
// instantiate the kernels through it.
#pragma once

#include <algorithm>
#include <utility>

#include "host/query_plan.hpp"   // query_grid
#include "query_kernel.hpp"

namespace rtw {

// Grid of a query or feature pass: `blocks` workgroups of work (a query: one per
// 256 rays; a feature pass: one wave per tile), no more than fit on the GPU at
// once for this kernel and LDS size -- a workgroup loops over ray blocks or takes
// tiles from a counter, so what it stages into LDS is paid once.  `grid_cap`:
// tuning "query_grid" (0: no cap), at most that many workgroups.
template <typename K>
inline uint32_t resident_grid(K kernel, uint64_t blocks, size_t lds_bytes, uint32_t grid_cap) {
    int per_cu = 0, dev = 0, cus = 0;
    uint64_t resident = 2048;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), (int)kQueryBlock,
                                                     lds_bytes) == hipSuccess &&
        hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per_cu >= 1 && cus >= 1)
        resident = (uint64_t)per_cu * cus;
    return query_grid(blocks, resident, grid_cap);
}

template <typename K, typename Params>
inline int launch_resident(K kernel, uint64_t blocks, const Params& p, size_t lds_bytes, uint32_t grid_cap,
                           hipStream_t stream) {
    // dynamic LDS above 64 KiB must be allowed per kernel
    if (lds_bytes > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes);
    hipLaunchKernelGGL(kernel, dim3(resident_grid(kernel, blocks, lds_bytes, grid_cap)), dim3(kQueryBlock), lds_bytes,
                       stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// A kernel table: entry I is Entry::run<I / 2, I % 2> -- <world or light path, robust>.
// Returns what the entry returns (the world / path launched, or -1), -1 without one.
template <typename Entry, typename Params, size_t... I>
inline int launch_table(const Params& p, int which, bool robust, size_t lds_bytes, uint32_t grid_cap,
                        hipStream_t stream, std::index_sequence<I...>) {
    int ran = -1;   // (no such entry)
    (void)((which == (int)I / 2 && robust == (I % 2 != 0) &&
            ((ran = Entry::template run<(int)I / 2, I % 2 != 0>(p, lds_bytes, grid_cap, stream)), true)) || ...);
    return ran;
}

template <typename R>
struct HitEntry {
    template <int kWorld, bool kRobust>
    static int run(const QParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (hit_kernel_exists(sizeof(R) == 8, kWorld, kRobust))
            return launch_resident(&dev::hit_rays_kernel<R, kWorld, kRobust>, (p.n + kQueryBlock - 1) / kQueryBlock, p,
                                   lds_bytes, grid_cap, stream) ? -1 : kWorld;
        else
            return -1;
    }
};
template <typename R>
struct LightEntry {
    template <int kPath, bool kRobust>
    static int run(const QParams<R>& p, size_t lds_bytes, uint32_t grid_cap, hipStream_t stream) {
        if constexpr (light_kernel_exists(sizeof(R) == 8, kPath, kRobust))
            return launch_resident(&dev::light_pdf_rays_kernel<R, kPath, kRobust>,
                                   (p.n + kQueryBlock - 1) / kQueryBlock, p, lds_bytes, grid_cap, stream) ? -1 : kPath;
        else
            return -1;
    }
};

// (defined by the unit of each precision)
#define RTW_QUERY_UNIT(R)                                                                                      \
    int launch_hit_rays(const QParams<R>& p, int world, bool robust, size_t lds_bytes, uint32_t grid_cap,      \
                        hipStream_t stream) {                                                                  \
        return launch_table<HitEntry<R>>(p, world, robust, lds_bytes, grid_cap, stream,                        \
                                         std::make_index_sequence<2 * (kWorldBvhLds + 1)>());                  \
    }                                                                                                          \
    int launch_light_pdf_rays(const QParams<R>& p, int path, bool robust, size_t lds_bytes, uint32_t grid_cap, \
                              hipStream_t stream) {                                                            \
        return launch_table<LightEntry<R>>(p, path, robust, lds_bytes, grid_cap, stream,                       \
                                           std::make_index_sequence<2 * kLightPaths>());                       \
    }

}  // namespace rtw
