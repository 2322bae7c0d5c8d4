// denoise_variance.cpp -- Camera::render_window_moments and
// rtw::denoise_variance of the C++ host mirror (rtw_host.hpp) through
// rtw_render_window_moments and rtw_denoise_variance.  Its own unit, as
// denoise.cpp: programs that link rtw_host.cpp without a device need no more
// entry points than Camera::render uses.
#include "rtw_host.hpp"

namespace rtw {

void Camera::render_window_moments(const HittableList& world, const HittableList& lights, uint32_t first, uint32_t n,
                                   std::vector<double>& sums, std::vector<double>& moments,
                                   const RenderOptions& opt) const {
    const size_t px = (size_t)c_.image_width * c_.image_height;
    if (first == 0) {
        sums.assign(px * 3, 0.0);
        moments.assign(px * 2, 0.0);
    }
    if (sums.size() != px * 3) throw Error(RTW_E_INVALID, "render_window_moments: sums holds 3 values per pixel");
    if (moments.size() != px * 2) throw Error(RTW_E_INVALID, "render_window_moments: moments holds 2 values per pixel");
    if (px == 0 || n == 0) return;
    FlatScene flat = flatten(world, lights);
    rtw_scene view = flat.view();
    rtw_ctx* ctx = create_context(opt);
    rtw_set_accel(ctx, opt.accel);
    int rc = rtw_set_scene(ctx, &view);
    if (rc == RTW_OK)
        rc = rtw_render_window_moments(ctx, &c_, opt.seed, first, n, sums.data(), moments.data(), nullptr);
    std::string err = rc ? rtw_last_error(ctx) : "";
    rtw_destroy(ctx);
    if (rc != RTW_OK) throw Error(rc, "rtw_render_window_moments: " + err);
}

std::vector<double> denoise_variance(const std::vector<double>& sums, const std::vector<double>& features,
                                     const std::vector<double>& moments, const std::vector<uint32_t>& counts,
                                     uint32_t spp, uint32_t width, uint32_t height,
                                     const rtw_denoise_variance_params* params, rtw_denoise_stats* stats,
                                     const RenderOptions& opt) {
    const size_t px = (size_t)width * height;
    if (sums.size() != px * 3) throw Error(RTW_E_INVALID, "denoise_variance: sums holds 3 values per pixel");
    if (features.size() != px * 8) throw Error(RTW_E_INVALID, "denoise_variance: features holds 8 values per pixel");
    if (moments.size() != px * 2) throw Error(RTW_E_INVALID, "denoise_variance: moments holds 2 values per pixel");
    if (!counts.empty() && counts.size() != px)
        throw Error(RTW_E_INVALID, "denoise_variance: counts holds one value per pixel");
    std::vector<double> out(px * 3, 0.0);
    if (px == 0) return out;
    rtw_ctx* ctx = create_context(opt);
    int rc = rtw_denoise_variance(ctx, sums.data(), features.data(), moments.data(),
                                  counts.empty() ? nullptr : counts.data(), spp, width, height, params, out.data());
    if (rc == RTW_OK && stats) rc = rtw_get_denoise_stats(ctx, stats);
    std::string err = rc ? rtw_last_error(ctx) : "";
    rtw_destroy(ctx);
    if (rc != RTW_OK) throw Error(rc, "rtw_denoise_variance: " + err);
    return out;
}

}  // namespace rtw
