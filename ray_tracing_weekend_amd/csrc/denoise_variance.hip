// denoise_variance.hip -- the kernels of rtw_denoise_variance
// (denoise_variance_kernels.hpp) and their launches.  Built with
// -ffp-contract=off, as denoise.hip: the filter is f64 arithmetic whose every
// operation rounds on its own; the sums' precision only says how the colour
// sums are read.
#define RTW_SVGF_KERNELS
#include "denoise_variance_kernels.hpp"

namespace rtw {

int launch_svgf_prepare(bool sums_f32, const SvgfPrepare& p, uint32_t blocks, hipStream_t stream) {
    if (blocks == 0) return 0;
    if (sums_f32) hipLaunchKernelGGL((dev::svgf_prepare_kernel<float>), dim3(blocks), dim3(kDenoiseBlock), 0, stream, p);
    else hipLaunchKernelGGL((dev::svgf_prepare_kernel<double>), dim3(blocks), dim3(kDenoiseBlock), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_svgf_atrous(const SvgfAtrous& p, const SvgfStep& s, hipStream_t stream) {
    if (s.grid_x == 0 || s.grid_y == 0) return 0;
    const dim3 grid(s.grid_x, s.grid_y), block(kDenoiseTileW, kDenoiseTileH);
    if (s.lds) {
        // dynamic LDS above 64 KiB must be allowed per kernel
        if (s.lds_bytes > 65536 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(&dev::svgf_atrous_kernel<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds_bytes) != hipSuccess)
            return -1;
        hipLaunchKernelGGL((dev::svgf_atrous_kernel<true>), grid, block, s.lds_bytes, stream, p);
    } else {
        hipLaunchKernelGGL((dev::svgf_atrous_kernel<false>), grid, block, 0, stream, p);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rtw
