// path_f64.hip -- parity-mode (f64) instantiation of camera_rays_kernel /
// shade_rays_kernel.  Built like query_f64.hip: -ffp-contract=off, the
// reference's operation order, bit-comparable with the oracle.
#include "path_launch.hpp"

namespace rtw {

RTW_PATH_UNIT(double)

}  // namespace rtw
