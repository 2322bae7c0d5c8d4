// direct_f32.hip -- f32 instantiation of direct_light_kernel.  Built like
// query_f32.hip: -ffp-contract=on, the f32 kernels' arithmetic; the sums stay f64.
#include "direct_launch.hpp"

namespace rtw {

RTW_DIRECT_UNIT(float)

}  // namespace rtw
