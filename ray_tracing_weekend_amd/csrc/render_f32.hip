// render_f32.hip -- speed-mode (f32) instantiation of the render kernels.
// Built with -ffp-contract=on (FMA within a source expression) and native
// sqrt/rcp/rsq/sin/cos.
#include "render_launch.hpp"

namespace rtw {

int launch_render(const KParams<float>& p, int world, int opts, size_t lds_bytes, const Fold<float>& fold,
                  hipStream_t stream, hipEvent_t mid) {
    return launch_render_impl<float>(p, world, opts, lds_bytes, fold, stream, mid);
}

template int launch_assemble<float>(const float*, size_t, uint32_t, uint32_t, uint32_t, const uint32_t*, float*,
                                   hipStream_t);

}  // namespace rtw
