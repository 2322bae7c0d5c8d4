// nee_f32.hip -- speed-mode (f32) instantiation of occlusion_kernel /
// light_sample_kernel.  Built like query_f32.hip: -ffp-contract=on, so the
// device functions round as in the f32 query and render kernels.
#include "nee_launch.hpp"

namespace rtw {

RTW_NEE_UNIT(float)

}  // namespace rtw
