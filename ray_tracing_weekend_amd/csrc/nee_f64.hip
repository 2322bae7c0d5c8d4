// nee_f64.hip -- parity-mode (f64) instantiation of occlusion_kernel /
// light_sample_kernel.  Built like query_f64.hip: -ffp-contract=off, the
// reference's operation order, bit-comparable with the oracle.
#include "nee_launch.hpp"

namespace rtw {

RTW_NEE_UNIT(double)

}  // namespace rtw
