// adaptive.hip -- the kernels of adaptive sampling (adaptive_kernels.hpp) and
// their launches.  Built with -ffp-contract=off for both precisions: the
// precision only says how the chunk sums are read; the statistic and the stop
// rule are f64 operations that round one by one, so an f32 context decides
// exactly as the rule is written.
#include "adaptive_kernels.hpp"

namespace rtw {

int launch_fold_adaptive(bool f64, const AdaptiveFold& f, hipStream_t stream) {
    if (f.n_active == 0) return 0;
    if (f64) hipLaunchKernelGGL((dev::fold_adaptive_kernel<double>), dim3(f.n_active), dim3(64), 0, stream, f);
    else hipLaunchKernelGGL((dev::fold_adaptive_kernel<float>), dim3(f.n_active), dim3(64), 0, stream, f);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_compact_tiles(const uint32_t* flags, uint32_t n_tiles, uint32_t W, uint32_t H, uint32_t* list,
                         uint32_t* meta, hipStream_t stream) {
    hipLaunchKernelGGL(dev::compact_tiles_kernel, dim3(1), dim3(256), 0, stream, flags, n_tiles, W, H, list, meta);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_unpack_adaptive(const double* sums, const uint32_t* counts, uint32_t W, uint32_t H, double* img,
                           uint32_t* img_counts, hipStream_t stream) {
    const uint64_t n_tiles = (uint64_t)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
    const uint32_t blocks = (uint32_t)((n_tiles * 64 + 255) / 256);
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(dev::unpack_adaptive_kernel, dim3(blocks), dim3(256), 0, stream, sums, counts, W, H,
                       (uint32_t)n_tiles, img, img_counts);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_pack_adaptive(const uint32_t* tiles, uint32_t n_tiles, const double* sums, const uint32_t* counts,
                         double* records, hipStream_t stream) {
    if (n_tiles == 0) return 0;
    hipLaunchKernelGGL(dev::pack_adaptive_kernel, dim3(n_tiles), dim3(64), 0, stream, tiles, sums, counts, records);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_assemble_adaptive(const double* ranks, size_t rank_stride, uint32_t nranks, uint32_t W, uint32_t H,
                             const uint32_t* slot, double* img, uint32_t* img_counts, hipStream_t stream) {
    const uint32_t tiles_x = (W + kTile - 1) / kTile, n_tiles = tiles_x * ((H + kTile - 1) / kTile);
    const uint32_t blocks = (uint32_t)(((uint64_t)n_tiles * 64 + 255) / 256);
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(dev::assemble_adaptive_kernel, dim3(blocks), dim3(256), 0, stream, ranks, rank_stride, nranks,
                       W, H, tiles_x, n_tiles, slot, img, img_counts);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rtw
