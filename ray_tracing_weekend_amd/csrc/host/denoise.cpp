// denoise.cpp -- rtw::denoise of the C++ host mirror (rtw_host.hpp) through
// rtw_denoise.  Its own unit, as render_features.cpp: programs that link
// rtw_host.cpp without a device need no more entry points than Camera::render
// uses.
#include "rtw_host.hpp"

namespace rtw {

std::vector<double> denoise(const std::vector<double>& sums, const std::vector<double>& features,
                            const std::vector<uint32_t>& counts, uint32_t spp, uint32_t width, uint32_t height,
                            const rtw_denoise_params* params, rtw_denoise_stats* stats, const RenderOptions& opt) {
    const size_t px = (size_t)width * height;
    if (sums.size() != px * 3) throw Error(RTW_E_INVALID, "denoise: sums holds 3 values per pixel");
    if (features.size() != px * 8) throw Error(RTW_E_INVALID, "denoise: features holds 8 values per pixel");
    if (!counts.empty() && counts.size() != px) throw Error(RTW_E_INVALID, "denoise: counts holds one value per pixel");
    std::vector<double> out(px * 3, 0.0);
    if (px == 0) return out;
    rtw_ctx* ctx = create_context(opt);
    int rc = rtw_denoise(ctx, sums.data(), features.data(), counts.empty() ? nullptr : counts.data(), spp, width,
                         height, params, out.data());
    if (rc == RTW_OK && stats) rc = rtw_get_denoise_stats(ctx, stats);
    std::string err = rc ? rtw_last_error(ctx) : "";
    rtw_destroy(ctx);
    if (rc != RTW_OK) throw Error(rc, "rtw_denoise: " + err);
    return out;
}

}  // namespace rtw
