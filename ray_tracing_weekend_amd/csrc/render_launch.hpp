// render_launch.hpp -- host side of the render kernels: the launch of the
// kernel variant a scene needs (launch_world), the chunk reduction after it
// and the tile assembly.  Included by the three .hip units, which instantiate
// the kernels through it.
#pragma once

#include "render_kernel.hpp"

namespace rtw {

// dynamic LDS above 64 KiB must be allowed per kernel
template <typename R, int kWorld, int kOpt>
inline void allow_lds(size_t lds_bytes) {
    if (lds_bytes > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&dev::render_kernel<R, kWorld, kOpt>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

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

constexpr int kVariantRan = 1 << 16;
// Launch the render kernel of `world` with options kOpt; returns the variant
// that ran as kVariantRan | (world << 8) | options (the brute-force worlds drop
// the light BVH, textured scenes map to the while-while BVH).
template <typename R, int kOpt>
inline int launch_world(const KParams<R>& p, int world, size_t lds_bytes, hipStream_t stream) {
    // the grid: one task per wave (p.persist 0), a fixed grid (p.persist), or the
    // resident workgroups (kPersistResident), in workgroups of the kernel's size
    auto grid = [&](uint32_t waves) {
        uint32_t b = (p.n_tasks + waves - 1) / waves;
        if (p.persist && p.persist != kPersistResident) b = b < p.persist ? b : p.persist;
        return b;
    };
    uint32_t blocks = 0;
    const size_t stacks = traversal_lds<R>(p.stack, (kOpt & dev::kOptLightBvh) != 0);
    const bool resident = p.persist == kPersistResident;
    constexpr int kBrute = kOpt & ~dev::kOptLightBvh;   // the light BVH needs the BVH kernels' stack
    // textured scenes are small: their kernels exist for the brute-force and
    // binary while-while worlds only (launch_render_impl maps the others)
    if constexpr ((kOpt & dev::kOptTex) != 0) {
        if (world == kWorldBvh4 || world == kWorldBvh) world = kWorldBvhWW;
    }
    // (the light BVH / grid is only chosen with a BVH world: its brute-force
    // cases are never reached, and instantiating them would put copies of the
    // plain brute-force kernels into the f64 light-grid unit)
    if constexpr ((kOpt & dev::kOptLightBvh) != 0) {
        if (world == kWorldLds || world == kWorldGlobal) return -1;
    }
    switch (world) {
    case kWorldLds:
        if constexpr ((kOpt & dev::kOptLightBvh) == 0) {
            allow_lds<R, kWorldLds, kBrute>(lds_bytes);
            blocks = grid(dev::kernel_waves<R, kWorldLds, kBrute>());
            if (resident) blocks = resident_blocks<R, kWorldLds, kBrute>(blocks, lds_bytes);
            hipLaunchKernelGGL((dev::render_kernel<R, kWorldLds, kBrute>), dim3(blocks),
                               dim3(64 * dev::kernel_waves<R, kWorldLds, kBrute>()), lds_bytes,
                               stream, p);
        }
        return kVariantRan | (kWorldLds << 8) | kBrute;
    case kWorldBvhLds:
        allow_lds<R, kWorldBvhLds, kOpt>(lds_bytes);
        blocks = grid(dev::kernel_waves<R, kWorldBvhLds, kOpt>());
        if (resident) blocks = resident_blocks<R, kWorldBvhLds, kOpt>(blocks, lds_bytes);
        hipLaunchKernelGGL((dev::render_kernel<R, kWorldBvhLds, kOpt>), dim3(blocks),
                           dim3(64 * dev::kernel_waves<R, kWorldBvhLds, kOpt>()), lds_bytes,
                           stream, p);
        return kVariantRan | (kWorldBvhLds << 8) | kOpt;
    case kWorldBvh4:
        if constexpr ((kOpt & dev::kOptTex) == 0) {
            blocks = grid(dev::kernel_waves<R, kWorldBvh4, kOpt>());
            if (resident) blocks = resident_blocks<R, kWorldBvh4, kOpt>(blocks, stacks);
            hipLaunchKernelGGL((dev::render_kernel<R, kWorldBvh4, kOpt>), dim3(blocks),
                               dim3(64 * dev::kernel_waves<R, kWorldBvh4, kOpt>()), stacks, stream, p);
        }
        return kVariantRan | (kWorldBvh4 << 8) | kOpt;
    case kWorldBvhWW:
        blocks = grid(dev::kernel_waves<R, kWorldBvhWW, kOpt>());
        if (resident) blocks = resident_blocks<R, kWorldBvhWW, kOpt>(blocks, stacks);
        hipLaunchKernelGGL((dev::render_kernel<R, kWorldBvhWW, kOpt>), dim3(blocks),
                           dim3(64 * dev::kernel_waves<R, kWorldBvhWW, kOpt>()), stacks,
                           stream, p);
        return kVariantRan | (kWorldBvhWW << 8) | kOpt;
    case kWorldBvh:
        if constexpr ((kOpt & dev::kOptTex) == 0) {
            blocks = grid(dev::kernel_waves<R, kWorldBvh, kOpt>());
            if (resident) blocks = resident_blocks<R, kWorldBvh, kOpt>(blocks, stacks);
            hipLaunchKernelGGL((dev::render_kernel<R, kWorldBvh, kOpt>), dim3(blocks),
                               dim3(64 * dev::kernel_waves<R, kWorldBvh, kOpt>()), stacks, stream, p);
        }
        return kVariantRan | (kWorldBvh << 8) | kOpt;
    default:
        if constexpr ((kOpt & dev::kOptLightBvh) == 0) {
            blocks = grid(dev::kernel_waves<R, kWorldGlobal, kBrute>());
            if (resident) blocks = resident_blocks<R, kWorldGlobal, kBrute>(blocks, 0);
            hipLaunchKernelGGL((dev::render_kernel<R, kWorldGlobal, kBrute>), dim3(blocks),
                               dim3(64 * dev::kernel_waves<R, kWorldGlobal, kBrute>()), 0, stream,
                               p);
        }
        return kVariantRan | (kWorldGlobal << 8) | kBrute;
    }
}

// The f64 kernels with the light BVH / grid are compiled in their own unit
// (render_f64_lgrid.hip) without the shared-divisor quotients (RTW_FASTDIV
// 0: C3 f64 +1.1 % with them, profiles/r06c3fd_ab.log); kOpt includes kOptLightBvh
int launch_render_f64_lgrid(const KParams<double>& p, int world, size_t lds_bytes, hipStream_t stream, int kopt);
// the f64 light-grid unit's body (instantiated there only)
template <typename R>
inline int launch_lgrid_impl(const KParams<R>& p, int world, size_t lds_bytes, hipStream_t stream, int kopt) {
    constexpr int T = dev::kOptTex | dev::kOptPrims, Pr = dev::kOptPrims, L = dev::kOptLightBvh;
    switch (kopt) {
    case T | L: return launch_world<R, T | L>(p, world, lds_bytes, stream);
    case Pr | L: return launch_world<R, Pr | L>(p, world, lds_bytes, stream);
    case L: return launch_world<R, L>(p, world, lds_bytes, stream);
    default: return -1;
    }
}

// Options per launch: the f32 sphere-test form (DevScene::robust; f64 keeps
// the reference arithmetic only) and the light BVH (KParams::light_bvh).
// Returns the variant that ran (launch_world's code; 0: no launch), or -1.
// `accum` non-null: a sample window -- fold_window_kernel onto accum (read when
// first_sample > 0; out may then be null) instead of the chunk reduction.
template <typename R>
inline int launch_render_impl(const KParams<R>& p_in, int world, size_t lds_bytes, R* out,
                              hipStream_t stream, hipEvent_t mid, double* accum = nullptr,
                              uint32_t first_sample = 0) {
    int ran = 0;
    // (a window: the render kernel's absolute view; the fold below reads p_in)
    const KParams<R> p = render_kernel_view(p_in);
    if (p.n_tasks) {
        const bool robust = sizeof(R) == 4 && p.sc.robust;
        const bool lbvh = p.light_bvh != 0;
        // kOptPrims: always for textured kernels; the Book-1 kernels go
        // without when the scene has no quads, cuboids, mixed list or
        // DiffuseLight (their emission accumulator is three bits, ResAcc)
        const bool prims = p.sc.n_quads || p.sc.n_boxes || p.sc.lref || p.sc.emissive;
        constexpr int T = dev::kOptTex | dev::kOptPrims, Pr = dev::kOptPrims;
        if (p.sc.mat_tex) {
            if constexpr (sizeof(R) == 4) {
                if (robust && lbvh) ran = launch_world<R, T | dev::kOptRobust | dev::kOptLightBvh>(p, world, lds_bytes, stream);
                else if (robust) ran = launch_world<R, T | dev::kOptRobust>(p, world, lds_bytes, stream);
                else if (lbvh) ran = launch_world<R, T | dev::kOptLightBvh>(p, world, lds_bytes, stream);
                else ran = launch_world<R, T>(p, world, lds_bytes, stream);
            } else {
                if (lbvh) ran = launch_render_f64_lgrid(p, world, lds_bytes, stream, T | dev::kOptLightBvh);
                else ran = launch_world<R, T>(p, world, lds_bytes, stream);
            }
        } else if constexpr (sizeof(R) == 4) {
            if (prims) {
                if (robust && lbvh) ran = launch_world<R, Pr | dev::kOptRobust | dev::kOptLightBvh>(p, world, lds_bytes, stream);
                else if (robust) ran = launch_world<R, Pr | dev::kOptRobust>(p, world, lds_bytes, stream);
                else if (lbvh) ran = launch_world<R, Pr | dev::kOptLightBvh>(p, world, lds_bytes, stream);
                else ran = launch_world<R, Pr>(p, world, lds_bytes, stream);
            } else {
                constexpr int H = dev::kOptHit64;
                if (p.hit64) {
                    if (robust && lbvh) ran = launch_world<R, H | dev::kOptRobust | dev::kOptLightBvh>(p, world, lds_bytes, stream);
                    else if (robust) ran = launch_world<R, H | dev::kOptRobust>(p, world, lds_bytes, stream);
                    else if (lbvh) ran = launch_world<R, H | dev::kOptLightBvh>(p, world, lds_bytes, stream);
                    else ran = launch_world<R, H>(p, world, lds_bytes, stream);
                } else {
                    if (robust && lbvh) ran = launch_world<R, dev::kOptRobust | dev::kOptLightBvh>(p, world, lds_bytes, stream);
                    else if (robust) ran = launch_world<R, dev::kOptRobust>(p, world, lds_bytes, stream);
                    else if (lbvh) ran = launch_world<R, dev::kOptLightBvh>(p, world, lds_bytes, stream);
                    else ran = launch_world<R, 0>(p, world, lds_bytes, stream);
                }
            }
        } else {
            // f64: the sphere + plane scenes' kernels go without the quad / cuboid code
            // too (156 instead of 176 VGPRs: 3 waves per SIMD instead of 2)
            (void)robust;
            if (prims) {
                if (lbvh) ran = launch_render_f64_lgrid(p, world, lds_bytes, stream, Pr | dev::kOptLightBvh);
                else ran = launch_world<R, Pr>(p, world, lds_bytes, stream);
            } else {
                if (lbvh) ran = launch_render_f64_lgrid(p, world, lds_bytes, stream, dev::kOptLightBvh);
                else ran = launch_world<R, 0>(p, world, lds_bytes, stream);
            }
        }
        if (hipGetLastError() != hipSuccess) return -1;
    }
    if (mid && hipEventRecord(mid, stream) != hipSuccess) return -1;
    if (p_in.n_local_tiles && accum) {
        hipLaunchKernelGGL((dev::fold_window_kernel<R>), dim3(p_in.n_local_tiles), dim3(64), 0, stream, p_in,
                           accum, first_sample, out);
        if (hipGetLastError() != hipSuccess) return -1;
    } else if (p_in.n_local_tiles) {
        hipLaunchKernelGGL((dev::reduce_chunks_kernel<R>), dim3(p_in.n_local_tiles), dim3(64), 0, stream, p_in,
                           out);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return ran;
}

template <typename R>
inline int launch_assemble_impl(const R* ranks, size_t rank_stride, uint32_t nranks, uint32_t W, uint32_t H,
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
