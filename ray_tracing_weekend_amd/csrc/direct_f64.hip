// direct_f64.hip -- parity-mode (f64) instantiation of direct_light_kernel.
// Built like query_f64.hip: -ffp-contract=off, the reference's operation order,
// bit-comparable with the independent restatement.
#include "direct_launch.hpp"

namespace rtw {

RTW_DIRECT_UNIT(double)

}  // namespace rtw
