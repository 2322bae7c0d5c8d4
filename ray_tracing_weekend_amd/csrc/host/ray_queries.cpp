// ray_queries.cpp -- hit_rays / light_pdf of the C++ host mirror (rtw_host.hpp):
// the batched Hittable::hit and light-list pdf_value through rtw_hit_rays /
// rtw_light_pdf_rays.  Its own unit, so that programs that link rtw_host.cpp
// without a device (the CPU checks) need no more entry points than
// Camera::render uses.
#include "rtw_host.hpp"

namespace rtw {

namespace {

// the staged scene of (world, lights) on one device, f64 (device_mask is not a query's)
rtw_ctx* query_context(const HittableList& world, const HittableList& lights, const RenderOptions& opt) {
    if (opt.precision != RTW_F64) throw Error(RTW_E_INVALID, "the C++ mirror's ray queries are f64 (RTW_F64)");
    RenderOptions one = opt;
    one.device_mask = 0;
    const FlatScene flat = flatten(world, lights);
    const rtw_scene view = flat.view();
    rtw_ctx* ctx = create_context(one);
    rtw_set_accel(ctx, opt.accel);
    const int rc = rtw_set_scene(ctx, &view);
    if (rc != RTW_OK) {
        const std::string err = rtw_last_error(ctx);
        rtw_destroy(ctx);
        throw Error(rc, "rtw_set_scene: " + err);
    }
    return ctx;
}

void finish(rtw_ctx* ctx, int rc, const char* what) {
    const std::string err = rc ? rtw_last_error(ctx) : "";
    rtw_destroy(ctx);
    if (rc != RTW_OK) throw Error(rc, std::string(what) + ": " + err);
}

}  // namespace

std::vector<RayHit> hit_rays(const HittableList& world, const HittableList& lights, const std::vector<double>& rays,
                             double t_min, const RenderOptions& opt) {
    if (rays.size() % 6) throw Error(RTW_E_INVALID, "hit_rays: rays holds 6 values per ray");
    const size_t n = rays.size() / 6;
    std::vector<double> hits(9 * n);
    std::vector<int32_t> ids(4 * n);
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_hit_rays(ctx, rays.data(), n, t_min, hits.data(), ids.data()), "rtw_hit_rays");
    std::vector<RayHit> out(n);
    for (size_t k = 0; k < n; ++k) {
        const double* h = &hits[9 * k];
        const int32_t* id = &ids[4 * k];
        out[k] = RayHit{h[0], {h[1], h[2], h[3]}, {h[4], h[5], h[6]}, h[7], h[8], id[0], id[1], id[2] != 0, id[3]};
    }
    return out;
}

std::vector<double> light_pdf(const HittableList& world, const HittableList& lights, const std::vector<double>& rays,
                              const RenderOptions& opt) {
    if (rays.size() % 6) throw Error(RTW_E_INVALID, "light_pdf: rays holds 6 values per (origin, direction)");
    const size_t n = rays.size() / 6;
    std::vector<double> pdf(n);
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_light_pdf_rays(ctx, rays.data(), n, pdf.data()), "rtw_light_pdf_rays");
    return pdf;
}

std::vector<uint8_t> occluded(const HittableList& world, const HittableList& lights, const std::vector<double>& rays,
                              const std::vector<double>& t_max, double t_min, const RenderOptions& opt) {
    if (rays.size() % 6) throw Error(RTW_E_INVALID, "occluded: rays holds 6 values per ray");
    const size_t n = rays.size() / 6;
    if (!t_max.empty() && t_max.size() != n) throw Error(RTW_E_INVALID, "occluded: t_max holds one value per ray");
    std::vector<uint8_t> occ(n);
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_occluded_rays(ctx, rays.data(), n, t_min, t_max.empty() ? nullptr : t_max.data(), occ.data()),
           "rtw_occluded_rays");
    return occ;
}

LightSamples light_sample(const HittableList& world, const HittableList& lights, const std::vector<double>& origins,
                          uint64_t seed, uint64_t first_stream, uint32_t sample, bool with_pdf,
                          const RenderOptions& opt) {
    if (origins.size() % 3) throw Error(RTW_E_INVALID, "light_sample: origins holds 3 values per point");
    const size_t n = origins.size() / 3;
    LightSamples out;
    out.directions.resize(3 * n);
    if (with_pdf) out.pdf.resize(n);
    out.light.resize(n);
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_light_sample(ctx, origins.data(), n, seed, first_stream, sample, out.directions.data(),
                                 with_pdf ? out.pdf.data() : nullptr, out.light.data()),
           "rtw_light_sample");
    return out;
}

}  // namespace rtw
