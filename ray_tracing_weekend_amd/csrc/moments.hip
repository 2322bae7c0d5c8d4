// moments.hip -- the kernels of the luminance moments (moments_kernels.hpp) and
// their launches.  Built with -ffp-contract=off for both precisions, as
// adaptive.hip: the precision only says how the chunk sums are read.
#define RTW_MOMENTS_KERNELS
#include "moments_kernels.hpp"

namespace rtw {

int launch_fold_moments(bool f64, const MomentsFold& f, hipStream_t stream) {
    if (f.n_tiles == 0) return 0;
    if (f64) hipLaunchKernelGGL((dev::fold_moments_kernel<double>), dim3(f.n_tiles), dim3(64), 0, stream, f);
    else hipLaunchKernelGGL((dev::fold_moments_kernel<float>), dim3(f.n_tiles), dim3(64), 0, stream, f);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_unpack_moments(const double* s12, uint32_t W, uint32_t H, double* img, hipStream_t stream) {
    const uint64_t n_tiles = (uint64_t)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile);
    const uint32_t blocks = (uint32_t)((n_tiles * 64 + 255) / 256);
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(dev::unpack_moments_kernel, dim3(blocks), dim3(256), 0, stream, s12, W, H, (uint32_t)n_tiles,
                       img);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rtw
