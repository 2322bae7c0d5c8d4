// radiance_f64.hip -- parity-mode (f64) instantiation of radiance_kernel.
// Built like query_f64.hip: -ffp-contract=off, the reference's operation order,
// bit-comparable with the independent restatement.
#include "radiance_launch.hpp"

namespace rtw {

RTW_RADIANCE_UNIT(double)

}  // namespace rtw
