// ray_queries.cpp -- hit_rays / light_pdf of the C++ host mirror (rtw_host.hpp):
// the batched Hittable::hit and light-list pdf_value through rtw_hit_rays /
// rtw_light_pdf_rays, the any-hit and light-sample queries, and the path queries
// (camera_rays / shade_rays through rtw_camera_rays / rtw_shade_rays) and the wavefront
// path rounds (path_advance / render_wavefront through rtw_path_advance /
// rtw_render_wavefront).  Its own unit, so that programs that link rtw_host.cpp
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

DirectLight direct_light(const HittableList& world, const HittableList& lights, const std::vector<double>& points,
                         uint64_t seed, uint32_t n_samples, uint64_t first_stream, uint32_t first_sample, double t_min,
                         bool records, const RenderOptions& opt) {
    if (points.size() % 6) throw Error(RTW_E_INVALID, "direct_light: points holds 6 values per point");
    const size_t n = points.size() / 6;
    DirectLight out;
    out.direct.resize(3 * n);
    if (records) {
        out.samples.resize(12 * n * n_samples);
        out.sample_ids.resize(4 * n * n_samples);
    }
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_direct_light(ctx, points.data(), n, seed, first_stream, first_sample, n_samples, t_min, 0,
                                 out.direct.data(), records && !out.samples.empty() ? out.samples.data() : nullptr,
                                 records && !out.sample_ids.empty() ? out.sample_ids.data() : nullptr),
           "rtw_direct_light");
    return out;
}

AmbientOcclusion ambient_occlusion(const HittableList& world, const HittableList& lights,
                                   const std::vector<double>& points, uint64_t seed, uint32_t n_samples, double t_max,
                                   double t_min, uint64_t first_stream, uint32_t first_sample, bool records,
                                   const RenderOptions& opt) {
    if (points.size() % 6) throw Error(RTW_E_INVALID, "ambient_occlusion: points holds 6 values per point");
    const size_t n = points.size() / 6;
    AmbientOcclusion out;
    out.open.resize(n);
    if (records) {
        out.directions.resize(3 * n * n_samples);
        out.occluded.resize(n * n_samples);
    }
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_ambient_occlusion(ctx, points.data(), n, seed, first_stream, first_sample, n_samples, t_min, t_max,
                                      0, out.open.data(), records && !out.directions.empty() ? out.directions.data() : nullptr,
                                      records && !out.occluded.empty() ? out.occluded.data() : nullptr),
           "rtw_ambient_occlusion");
    return out;
}

CameraRays camera_rays(const Camera& cam, uint64_t seed, uint32_t sample, const std::vector<uint32_t>& pixels,
                       uint64_t first_pixel, uint64_t n, const RenderOptions& opt) {
    if (opt.precision != RTW_F64) throw Error(RTW_E_INVALID, "the C++ mirror's ray queries are f64 (RTW_F64)");
    if (!pixels.empty()) n = pixels.size();
    CameraRays out;
    out.rays.resize(6 * n);
    out.rng.resize(4 * n);
    RenderOptions one = opt;
    one.device_mask = 0;
    rtw_ctx* ctx = create_context(one);   // (camera rays need no staged scene)
    finish(ctx, rtw_camera_rays(ctx, &cam.raw(), seed, sample, pixels.empty() ? nullptr : pixels.data(), first_pixel, n,
                                out.rays.data(), out.rng.data()),
           "rtw_camera_rays");
    return out;
}

Bounces shade_rays(const HittableList& world, const HittableList& lights, const std::vector<double>& rays,
                   const std::vector<RayHit>& hits, std::vector<uint64_t>& rng, bool with_pdfs,
                   const RenderOptions& opt) {
    if (rays.size() % 6) throw Error(RTW_E_INVALID, "shade_rays: rays holds 6 values per ray");
    const size_t n = rays.size() / 6;
    if (hits.size() != n || rng.size() != 4 * n)
        throw Error(RTW_E_INVALID, "shade_rays: one hit record and 4 rng words per ray");
    std::vector<double> h(9 * n);
    std::vector<int32_t> ids(4 * n);
    for (size_t k = 0; k < n; ++k) {
        const RayHit& r = hits[k];
        const double row[9] = {r.t, r.p.x, r.p.y, r.p.z, r.normal.x, r.normal.y, r.normal.z, r.u, r.v};
        for (int q = 0; q < 9; ++q) h[9 * k + q] = row[q];
        ids[4 * k] = r.object, ids[4 * k + 1] = r.material, ids[4 * k + 2] = r.front_face ? 1 : 0, ids[4 * k + 3] = r.kind;
    }
    Bounces out;
    out.next.resize(6 * n);
    out.weight.resize(3 * n);
    out.emitted.resize(3 * n);
    out.event.resize(n);
    if (with_pdfs) out.pdfs.resize(3 * n);
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_shade_rays(ctx, rays.data(), h.data(), ids.data(), n, rng.data(), out.next.data(), out.weight.data(),
                               out.emitted.data(), out.event.data(), with_pdfs ? out.pdfs.data() : nullptr),
           "rtw_shade_rays");
    return out;
}

PathState path_begin(const CameraRays& from, uint32_t first_slot) {
    const size_t n = from.rays.size() / 6;
    if ((uint64_t)first_slot + n > (uint64_t)1 << 32) throw Error(RTW_E_INVALID, "path_begin: first_slot + n is beyond 2^32 slots");
    PathState st;
    st.rays = from.rays;
    st.rng = from.rng;
    st.mult.assign(3 * n, 1.0);
    st.res.assign(3 * n, 0.0);
    st.slot.resize(n);
    for (size_t k = 0; k < n; ++k) st.slot[k] = first_slot + (uint32_t)k;
    return st;
}

PathState path_advance(const PathState& state, const Bounces& round, const std::vector<uint64_t>& rng,
                       std::vector<double>& colour, const Colour& background, bool last, const RenderOptions& opt) {
    if (opt.precision != RTW_F64) throw Error(RTW_E_INVALID, "the C++ mirror's ray queries are f64 (RTW_F64)");
    const size_t n = state.slot.size();
    if (state.mult.size() != 3 * n || state.res.size() != 3 * n || round.event.size() != n || round.weight.size() != 3 * n ||
        round.emitted.size() != 3 * n || round.next.size() != 6 * n || rng.size() != 4 * n || colour.size() % 3)
        throw Error(RTW_E_INVALID, "path_advance: the state's and the round's arrays hold one row per path, colour 3 per slot");
    PathState out;
    out.rays.resize(6 * n);
    out.rng.resize(4 * n);
    out.mult.resize(3 * n);
    out.res.resize(3 * n);
    out.slot.resize(n);
    const double bg[3] = {background.x, background.y, background.z};
    uint64_t m = 0;
    RenderOptions one = opt;
    one.device_mask = 0;
    rtw_ctx* ctx = create_context(one);   // (an advance needs no staged scene)
    finish(ctx, rtw_path_advance(ctx, n, state.mult.data(), state.res.data(), state.slot.data(), round.event.data(),
                                 round.weight.data(), round.emitted.data(), round.next.data(), rng.data(), out.rays.data(),
                                 out.rng.data(), out.mult.data(), out.res.data(), out.slot.data(), colour.data(),
                                 colour.size() / 3, bg, last ? 1 : 0, &m),
           "rtw_path_advance");
    out.rays.resize(6 * m);
    out.rng.resize(4 * m);
    out.mult.resize(3 * m);
    out.res.resize(3 * m);
    out.slot.resize(m);
    return out;
}

std::vector<double> render_wavefront(const Camera& cam, const HittableList& world, const HittableList& lights,
                                     uint64_t seed, uint32_t first_sample, uint32_t n_samples, uint32_t batch,
                                     std::vector<double> sums, const RenderOptions& opt) {
    const size_t len = (size_t)cam.raw().image_width * cam.raw().image_height * 3;
    if (sums.empty()) sums.assign(len, 0.0);
    if (sums.size() != len) throw Error(RTW_E_INVALID, "render_wavefront: sums holds H x W x 3 values");
    rtw_ctx* ctx = query_context(world, lights, opt);
    finish(ctx, rtw_render_wavefront(ctx, &cam.raw(), seed, first_sample, n_samples, batch, sums.data()),
           "rtw_render_wavefront");
    return sums;
}

}  // namespace rtw
