// render_features.cpp -- Camera::render_features of the C++ host mirror
// (rtw_host.hpp) through rtw_render_features.  Its own unit, as
// render_adaptive.cpp: programs that link rtw_host.cpp without a device need
// no more entry points than Camera::render uses.
#include "rtw_host.hpp"

namespace rtw {

std::vector<double> Camera::render_features(const HittableList& world, const HittableList& lights, uint32_t first,
                                            uint32_t n, const std::vector<uint32_t>& counts,
                                            std::vector<int32_t>* ids, const RenderOptions& opt) const {
    const uint32_t W = c_.image_width, H = c_.image_height;
    const size_t px = (size_t)W * H;
    if (!counts.empty() && counts.size() != px)
        throw Error(RTW_E_INVALID, "render_features: counts holds one value per pixel");
    if (opt.device_mask) throw Error(RTW_E_UNSUPPORTED, "render_features: one device");
    if (n == 0) n = c_.samples_per_pixel > first ? c_.samples_per_pixel - first : 0;
    FlatScene flat = flatten(world, lights);
    rtw_scene view = flat.view();
    rtw_ctx* ctx = create_context(opt);
    rtw_set_accel(ctx, opt.accel);
    int rc = rtw_set_scene(ctx, &view);
    std::vector<double> features(px * 8, 0.0);
    if (ids) ids->assign(px * 2, 0);
    if (rc == RTW_OK)
        rc = rtw_render_features(ctx, &c_, opt.seed, first, n, counts.empty() ? nullptr : counts.data(),
                                 features.data(), ids ? ids->data() : nullptr);
    std::string err = rc ? rtw_last_error(ctx) : "";
    rtw_destroy(ctx);
    if (rc != RTW_OK) throw Error(rc, "rtw_render_features: " + err);
    return features;
}

}  // namespace rtw
