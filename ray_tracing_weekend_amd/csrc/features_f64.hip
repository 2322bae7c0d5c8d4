// features_f64.hip -- parity-mode (f64) instantiation of the feature kernels.
// Built like render_f64.hip and query_f64.hip: -ffp-contract=off, the
// reference's operation order, bit-comparable with the oracle.
#include "features_launch.hpp"

namespace rtw {

RTW_FEATURES_UNIT(double)

}  // namespace rtw
