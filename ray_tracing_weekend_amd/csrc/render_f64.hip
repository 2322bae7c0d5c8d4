// render_f64.hip -- parity-mode (f64) instantiation of the render kernels.
// Built with -ffp-contract=off: every a*b+c rounds twice, in the reference's
// operation order, so the output is bit-comparable with the CPU oracle.
#include "render_launch.hpp"

namespace rtw {

int launch_render_f64(const KParams<double>& p, int world, int opts, size_t lds_bytes, double* out,
                      hipStream_t stream, hipEvent_t mid, double* accum, uint32_t first_sample) {
    return launch_render_impl<double>(p, world, opts, lds_bytes, out, stream, mid, accum, first_sample);
}

int launch_render_only_f64(const KParams<double>& p, int world, int opts, size_t lds_bytes, hipStream_t stream,
                           hipEvent_t mid) {
    return launch_render_impl<double>(p, world, opts, lds_bytes, nullptr, stream, mid, nullptr, 0, false);
}

int launch_assemble_f64(const double* ranks, size_t rank_stride, uint32_t nranks, uint32_t W, uint32_t H,
                        const uint32_t* slot, double* img, hipStream_t stream) {
    return launch_assemble_impl<double>(ranks, rank_stride, nranks, W, H, slot, img, stream);
}

}  // namespace rtw
