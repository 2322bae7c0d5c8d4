// ambient_f32.hip -- f32 instantiation of ambient_kernel.  Built like
// nee_f32.hip: -ffp-contract=on, the f32 kernels' arithmetic; the counts are integers.
#include "ambient_launch.hpp"

namespace rtw {

RTW_AMBIENT_UNIT(float)

}  // namespace rtw
