// query_f32.hip -- speed-mode (f32) instantiation of the ray-query kernels.
// Built like render_f32.hip: -ffp-contract=on, so every shared device function
// rounds here as it does in the f32 render kernels.
#include "query_launch.hpp"

namespace rtw {

RTW_QUERY_UNIT(float)

}  // namespace rtw
