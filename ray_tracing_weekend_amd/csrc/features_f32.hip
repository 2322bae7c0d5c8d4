// features_f32.hip -- speed-mode (f32) instantiation of the feature kernels.
// Built like render_f32.hip and query_f32.hip: -ffp-contract=on, so every
// shared device function rounds here as it does in the f32 query kernels.
#include "features_launch.hpp"

namespace rtw {

RTW_FEATURES_UNIT(float)

}  // namespace rtw
