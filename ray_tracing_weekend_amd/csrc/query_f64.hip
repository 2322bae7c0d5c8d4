// query_f64.hip -- parity-mode (f64) instantiation of the ray-query kernels.
// Built like render_f64.hip: -ffp-contract=off, the reference's operation
// order, bit-comparable with the oracle.
#include "query_launch.hpp"

namespace rtw {

RTW_QUERY_UNIT(double)

}  // namespace rtw
