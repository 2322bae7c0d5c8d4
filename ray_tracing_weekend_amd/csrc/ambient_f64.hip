// ambient_f64.hip -- parity-mode (f64) instantiation of ambient_kernel.
// Built like nee_f64.hip: -ffp-contract=off, the reference's operation order,
// bit-comparable with the independent restatement.
#include "ambient_launch.hpp"

namespace rtw {

RTW_AMBIENT_UNIT(double)

}  // namespace rtw
