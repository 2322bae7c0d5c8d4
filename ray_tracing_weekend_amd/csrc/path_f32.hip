// path_f32.hip -- speed-mode (f32) instantiation of camera_rays_kernel /
// shade_rays_kernel.  Built like query_f32.hip: -ffp-contract=on, the plain f32
// arithmetic of the f32 kernels.
#include "path_launch.hpp"

namespace rtw {

RTW_PATH_UNIT(float)

}  // namespace rtw
