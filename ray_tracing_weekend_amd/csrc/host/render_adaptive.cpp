// render_adaptive.cpp -- Camera::render_adaptive of the C++ host mirror
// (rtw_host.hpp) through rtw_render_adaptive_image; the pass plan and the stop rule
// are render_adaptive.hpp's.  Its own unit, as render_windows.cpp: programs
// that link rtw_host.cpp without a device need no more entry points than
// Camera::render uses.
#include "render_adaptive.hpp"

#include "rtw_host.hpp"

namespace rtw {

std::vector<std::vector<SampledColour>> Camera::render_adaptive(const HittableList& world,
                                                                const HittableList& lights, uint32_t min_samples,
                                                                uint32_t max_samples, uint32_t window,
                                                                double tolerance, const RenderOptions& opt) const {
    if (const char* why = adaptive_check(min_samples, max_samples, window, tolerance, 0))
        throw Error(RTW_E_INVALID, std::string("render_adaptive: ") + why);
    FlatScene flat = flatten(world, lights);
    rtw_scene view = flat.view();
    rtw_ctx* ctx = create_context(opt);
    rtw_set_accel(ctx, opt.accel);
    int rc = rtw_set_scene(ctx, &view);
    const uint32_t W = c_.image_width, H = c_.image_height;
    std::vector<double> sums((size_t)W * H * 3, 0.0);
    std::vector<uint32_t> counts((size_t)W * H, 0);
    if (rc == RTW_OK)
        rc = rtw_render_adaptive_image(ctx, &c_, opt.seed, min_samples, max_samples, window, tolerance, sums.data(),
                                 counts.data(), nullptr);
    std::string err = rc ? rtw_last_error(ctx) : "";
    rtw_destroy(ctx);
    if (rc != RTW_OK) throw Error(rc, "rtw_render_adaptive_image: " + err);
    std::vector<std::vector<SampledColour>> out(H, std::vector<SampledColour>(W));
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            const double* s = &sums[((size_t)j * W + i) * 3];
            out[j][i] = SampledColour{{s[0], s[1], s[2]}, (int32_t)counts[(size_t)j * W + i]};
        }
    return out;
}

}  // namespace rtw
