// render_launch.hpp -- host side of the render kernels: a table of the kernel
// variants this unit holds (launch_variant: no decision is made here -- the
// variant, its world, options and dynamic LDS, is host/render_plan.cpp's),
// the chunk reduction after the render kernel and the tile assembly.
// Included by the three .hip units, which instantiate the kernels through it.
#pragma once

#include <utility>

#include "render_kernel.hpp"

namespace rtw {

// Grid of a persistent launch (KParams::persist == kPersistResident): the
// workgroups that fit on the GPU at once for this kernel and LDS size (its
// occupancy x CUs), no more than the tasks need.  More than that only adds
// workgroups that start late and stretch the tail (C2 8-rank share: 2048
// workgroups 15.3 ms, 1024 = resident at 4 waves/SIMD 14.9 ms); co-residency
// is not required (no grid barrier: tasks come from a counter).
template <typename R, int kWorld, int kOpt>
inline uint32_t resident_blocks(uint32_t blocks, size_t lds_bytes) {
    int per_cu = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, reinterpret_cast<const void*>(&dev::render_kernel<R, kWorld, kOpt>),
            64 * dev::kernel_waves<R, kWorld, kOpt>(), lds_bytes) !=
            hipSuccess ||
        hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 ||
        cus < 1)
        return std::min<uint32_t>(blocks, 2048u);
    return std::min<uint32_t>(blocks, (uint32_t)(per_cu * cus));
}

// Launch render_kernel<R, kWorld, kOpt> with lds_bytes of dynamic LDS; returns
// the variant_code of this instantiation.
template <typename R, int kWorld, int kOpt>
inline int launch_one(const KParams<R>& p, size_t lds_bytes, hipStream_t stream) {
    constexpr uint32_t waves = dev::kernel_waves<R, kWorld, kOpt>();
    // dynamic LDS above 64 KiB must be allowed per kernel
    if (lds_bytes > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dev::render_kernel<R, kWorld, kOpt>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    // the grid: one task per wave (p.persist 0), a fixed grid (p.persist), or the
    // resident workgroups (kPersistResident), in workgroups of the kernel's size
    uint32_t blocks = (p.n_tasks + waves - 1) / waves;
    if (p.persist == kPersistResident) blocks = resident_blocks<R, kWorld, kOpt>(blocks, lds_bytes);
    else if (p.persist) blocks = std::min(blocks, p.persist);
    hipLaunchKernelGGL((dev::render_kernel<R, kWorld, kOpt>), dim3(blocks), dim3(64 * waves), lds_bytes, stream, p);
    return variant_code(kWorld, kOpt);
}

// The table: entry I is the variant <I / kOpts, I % kOpts>, present when it
// exists (rtw_kernels.h variant_exists) and belongs to this unit.  The f64
// kernels with the light BVH / grid (kLgrid) are compiled in their own unit
// (render_f64_lgrid.hip) without the shared-divisor quotients (RTW_FASTDIV 0:
// C3 f64 +1.1 % with them, profiles/r06c3fd_ab.log).
constexpr int kOpts = dev::kOptAll + 1, kVariants = (kWorldBvhLds + 1) * kOpts;
template <typename R, bool kLgrid, int kWorld, int kOpt>
inline int launch_entry(const KParams<R>& p, size_t lds_bytes, hipStream_t stream) {
    if constexpr (dev::variant_exists(sizeof(R) == 8, kWorld, kOpt) &&
                  (sizeof(R) == 8 && (kOpt & dev::kOptLightBvh) != 0) == kLgrid)
        return launch_one<R, kWorld, kOpt>(p, lds_bytes, stream);
    else
        return -1;
}
template <typename R, bool kLgrid, size_t... I>
inline int launch_variant(const KParams<R>& p, int world, int opts, size_t lds_bytes, hipStream_t stream,
                          std::index_sequence<I...>) {
    int ran = -1;   // (no such entry)
    (void)((world == (int)I / kOpts && opts == (int)I % kOpts &&
            ((ran = launch_entry<R, kLgrid, (int)I / kOpts, (int)I % kOpts>(p, lds_bytes, stream)), true)) || ...);
    return ran;
}
// the f64 light-grid unit's table (render_f64_lgrid.hip)
int launch_render_f64_lgrid(const KParams<double>& p, int world, int opts, size_t lds_bytes, hipStream_t stream);

// The render kernel <world, opts>, then the fold (rtw_kernels.h Fold).  Returns
// the variant that ran (launch_one's code; 0: no launch), or -1.
template <typename R>
inline int launch_render_impl(const KParams<R>& p_in, int world, int opts, size_t lds_bytes, const Fold<R>& fold,
                              hipStream_t stream, hipEvent_t mid) {
    int ran = 0;
    if (p_in.n_tasks) {
        // (a window: the render kernel's absolute view; the fold below reads p_in)
        const KParams<R> p = render_kernel_view(p_in);
        bool lgrid = false;   // f64 with the light BVH / grid: the other unit's table
        if constexpr (sizeof(R) == 8) {
            lgrid = (opts & dev::kOptLightBvh) != 0;
            if (lgrid) ran = launch_render_f64_lgrid(p, world, opts, lds_bytes, stream);
        }
        if (!lgrid) ran = launch_variant<R, false>(p, world, opts, lds_bytes, stream, std::make_index_sequence<kVariants>());
        if (ran < 0 || hipGetLastError() != hipSuccess) return -1;
    }
    if (mid && hipEventRecord(mid, stream) != hipSuccess) return -1;
    if (fold.kind == kFoldNone || !p_in.n_local_tiles) return ran;
    if (fold.kind == kFoldWindow)
        hipLaunchKernelGGL((dev::fold_window_kernel<R>), dim3(p_in.n_local_tiles), dim3(64), 0, stream, p_in,
                           fold.accum, fold.first_sample, fold.out, fold.cull);
    else
        hipLaunchKernelGGL((dev::reduce_chunks_kernel<R>), dim3(p_in.n_local_tiles), dim3(64), 0, stream, p_in,
                           fold.out, fold.cull);
    return hipGetLastError() != hipSuccess ? -1 : ran;
}

// (explicitly instantiated by the unit of each precision)
template <typename R>
int launch_assemble(const R* ranks, size_t rank_stride, uint32_t nranks, uint32_t W, uint32_t H,
                    const uint32_t* slot, R* img, hipStream_t stream) {
    const uint32_t tiles_x = (W + kTile - 1) / kTile, n_tiles = tiles_x * ((H + kTile - 1) / kTile);
    const uint32_t blocks = (uint32_t)(((uint64_t)n_tiles * 64 + 255) / 256);
    if (blocks) {
        hipLaunchKernelGGL((dev::assemble_tiles_kernel<R>), dim3(blocks), dim3(256), 0, stream, ranks, rank_stride,
                           nranks, W, H, tiles_x, n_tiles, slot, img);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

}  // namespace rtw
