// camera_params.hpp -- the camera as a kernel sees it: the fields KParams
// (a render pass, render_pass.hpp pass_params) and FParams (the feature pass,
// query_plan.hpp feature_params) share by name, filled from an rtw_camera in
// one place, so that both kernels start the same primary rays.  Host only, no
// HIP call.
#pragma once

#include <math.h>

#include "../../../include/rtw.h"

namespace rtw {

// P: KParams<R> or FParams<R>
template <typename R, typename P>
inline void fill_camera(P& p, const rtw_camera& cam) {
    for (int a = 0; a < 3; ++a) {
        p.center[a] = (R)cam.center[a];
        p.p00[a] = (R)cam.pixel00_loc[a];
        p.du[a] = (R)cam.pixel_delta_u[a];
        p.dv[a] = (R)cam.pixel_delta_v[a];
        p.disk_u[a] = (R)cam.defocus_disk_u[a];
        p.disk_v[a] = (R)cam.defocus_disk_v[a];
        p.bg[a] = (R)cam.background[a];
    }
    // Uniform::new_inclusive(-0.5, 0.5) scale (rand 0.8.6)
    const double max_rand = 1.0 - 2.220446049250313080847e-16;
    double scale = (0.5 - -0.5) / max_rand;
    while (scale * max_rand + -0.5 > 0.5) scale = nextafter(scale, 0.0);
    p.u_scale = (R)scale;
    p.defocus = cam.defocus_angle > 2.220446049250313080847e-16 ? 1u : 0u;
}

}  // namespace rtw
