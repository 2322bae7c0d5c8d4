// render_windows.cpp -- Camera::render_windows of the C++ host mirror
// (rtw_host.hpp): the progressive render through rtw_render_window_image.  Its own
// unit, so that programs that link rtw_host.cpp without a device (the CPU
// checks) need no more entry points than Camera::render uses.
#include <algorithm>

#include "rtw_host.hpp"

namespace rtw {

std::vector<std::vector<SampledColour>> Camera::render_windows(
    const HittableList& world, const HittableList& lights, uint32_t window,
    const std::function<bool(uint32_t, const std::vector<double>&)>& on_window, const RenderOptions& opt) const {
    if (window == 0) throw Error(RTW_E_INVALID, "render_windows: window must be >= 1");
    FlatScene flat = flatten(world, lights);
    rtw_scene view = flat.view();
    rtw_ctx* ctx = create_context(opt);
    rtw_set_accel(ctx, opt.accel);
    int rc = rtw_set_scene(ctx, &view);
    const uint32_t W = c_.image_width, H = c_.image_height, spp = c_.samples_per_pixel;
    std::vector<double> sums((size_t)W * H * 3, 0.0);
    uint32_t done = 0;
    while (rc == RTW_OK && done < spp) {
        const uint32_t n = std::min(window, spp - done);
        rc = rtw_render_window_image(ctx, &c_, opt.seed, done, n, sums.data(), nullptr);
        if (rc != RTW_OK) break;
        done += n;
        if (on_window && !on_window(done, sums)) break;
    }
    std::string err = rc ? rtw_last_error(ctx) : "";
    rtw_destroy(ctx);
    if (rc != RTW_OK) throw Error(rc, "rtw_render_window_image: " + err);
    std::vector<std::vector<SampledColour>> out(H, std::vector<SampledColour>(W));
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const double* s = &sums[((size_t)j * W + i) * 3];
            out[j][i] = SampledColour{{s[0], s[1], s[2]}, (int32_t)done};
        }
    return out;
}

}  // namespace rtw
