// radiance_f32.hip -- f32 instantiation of radiance_kernel.  Built like
// query_f32.hip: -ffp-contract=on, the f32 kernels' arithmetic; the sums stay f64.
#include "radiance_launch.hpp"

namespace rtw {

RTW_RADIANCE_UNIT(float)

}  // namespace rtw
