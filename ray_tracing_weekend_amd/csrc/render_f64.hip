// render_f64.hip -- parity-mode (f64) instantiation of the render kernels.
// Built with -ffp-contract=off: every a*b+c rounds twice, in the reference's
// operation order, so the output is bit-comparable with the CPU oracle.
#include "render_launch.hpp"

namespace rtw {

int launch_render(const KParams<double>& p, int world, int opts, size_t lds_bytes, const Fold<double>& fold,
                  hipStream_t stream, hipEvent_t mid) {
    return launch_render_impl<double>(p, world, opts, lds_bytes, fold, stream, mid);
}

template int launch_assemble<double>(const double*, size_t, uint32_t, uint32_t, uint32_t, const uint32_t*, double*,
                                   hipStream_t);

}  // namespace rtw
