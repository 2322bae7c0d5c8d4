// capi_radiance.cpp -- radiance along arbitrary rays as one query of the C-ABI
// (include/rtw.h): rtw_radiance_rays and its device form.  As the other queries
// (capi_query.cpp, capi_direct.cpp): checks (host/radiance_plan.hpp) -> plan
// (host/query_plan.hpp, the closest hit's and the light pdf's) -> params -> launch
// -> bookkeeping, on the query state's counters, events and staging buffers.
#include <limits>
#include <string>

#include "capi_ctx.hpp"
#include "host/radiance_plan.hpp"
#include "radiance_kernels.h"

namespace {

// what every query refuses before anything else (capi_query.cpp query_checks), what
// rtw_shade_rays refuses (capi_path.cpp shade_checks), then the arguments
// (host/radiance_plan.hpp)
int radiance_checks(rtw_ctx* c, const rtw::RadianceArgs& a) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    const bool f64 = c->precision != RTW_F32;
    const uint32_t n_list = f64 ? c->sc64.n_list : c->sc32.n_list;
    if (n_list == 0 && c->has_lambertian)
        return fail(c, RTW_E_NO_LIGHTS, "rtw_radiance_rays: the light list is empty and the scene holds a Lambertian "
                                        "material (the reference panics, hittable_list.rs:417)");
    const char* text = "";
    const int rc = rtw::radiance_check(a, f64, &text);
    return rc ? fail(c, rc, text) : RTW_OK;
}

struct RadianceCall {
    const void* rays;
    uint64_t n, seed, first_stream;
    uint32_t first_sample, n_samples, max_depth;
    const double* background;
    uint64_t* rng;
    int accumulate;
    double* radiance;
    void* colours;
    uint32_t* segments;
};

template <typename R>
int radiance_device_t(rtw_ctx* c, const RadianceCall& a, hipStream_t stream) {
    const rtw::DevScene<R>& sc = dev_scene<R>(c);
    const rtw::QueryPlan pl = rtw::plan_query<R>(c->knobs, sc, c->scale);
    if (pl.err) return fail(c, pl.err, pl.err_text);
    const rtw::RadiancePlan rp = rtw::plan_radiance(pl, sizeof(R) == 8);
    if (rp.err) return fail(c, rp.err, rp.err_text);
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::RParams<R> p{};
    p.sc = sc;
    p.sc.robust = pl.robust;
    p.rays = reinterpret_cast<const R*>(a.rays);
    p.radiance = a.radiance;
    p.colours = reinterpret_cast<R*>(a.colours);
    p.segments = a.segments;
    p.rng = a.rng;
    p.seed = a.seed;
    p.first_stream = a.first_stream;
    p.first_sample = a.first_sample;
    p.n_samples = a.n_samples;
    p.max_depth = a.max_depth;
    p.accumulate = a.accumulate ? 1u : 0u;
    p.light_path = pl.light_path;
    p.counters = q->d_counters;
    p.n = a.n;
    p.tmin = (R)std::numeric_limits<double>::epsilon();
    for (int k = 0; k < 3; ++k) p.bg[k] = (R)a.background[k];
    p.stack = pl.stack;
    p.light_stack = pl.light_stack;
    p.light_off = rp.light_off;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    const int ran = rtw::launch_radiance(p, pl.world, pl.robust != 0, rp.lds, c->knobs.query_grid, stream);
    if (ran >= 0 && ran != pl.world) return fail(c, RTW_E_DEVICE, "the launched query kernel is not the plan's");
    if (ran < 0)
        return fail(c, RTW_E_DEVICE, std::string("query kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.kernel = (uint32_t)ran;
    q->last.is_light_pdf = rtw::kQueryRadiance;
    q->any = true;
    return RTW_OK;
}

}  // namespace

extern "C" {

int rtw_radiance_rays_device(rtw_ctx* c, const void* d_rays, size_t rays_bytes, uint64_t n, uint64_t seed,
                             uint64_t first_stream, uint32_t first_sample, uint32_t n_samples, uint32_t max_depth,
                             const double background[3], uint64_t* d_rng, size_t rng_bytes, int accumulate,
                             double* d_radiance, size_t radiance_bytes, void* d_colours, size_t colours_bytes,
                             uint32_t* d_segments, size_t segments_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    rtw::RadianceArgs a;
    a.rays = d_rays, a.n = n, a.first_sample = first_sample, a.n_samples = n_samples;
    a.background = background, a.rng = d_rng, a.radiance = d_radiance;
    a.colours = d_colours, a.segments = d_segments;
    a.device = true;
    a.rays_bytes = rays_bytes, a.rng_bytes = rng_bytes, a.radiance_bytes = radiance_bytes;
    a.colours_bytes = colours_bytes, a.segments_bytes = segments_bytes;
    int rc = radiance_checks(c, a);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const RadianceCall call{d_rays, n, seed, first_stream, first_sample, n_samples, max_depth, background,
                            d_rng, accumulate, d_radiance, d_colours, d_segments};
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) { return radiance_device_t<decltype(r)>(c, call, s); });
}

int rtw_radiance_rays(rtw_ctx* c, const void* rays, uint64_t n, uint64_t seed, uint64_t first_stream,
                      uint32_t first_sample, uint32_t n_samples, uint32_t max_depth, const double background[3],
                      uint64_t* rng, int accumulate, double* radiance, void* colours, uint32_t* segments) {
    if (!c) return RTW_E_INVALID;
    rtw::RadianceArgs a;
    a.rays = rays, a.n = n, a.first_sample = first_sample, a.n_samples = n_samples;
    a.background = background, a.rng = rng, a.radiance = radiance;
    a.colours = colours, a.segments = segments;
    int rc = radiance_checks(c, a);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: rays | sums | rng in the queries' ray buffer (each part from a 16-byte
    // boundary), the colours in their record buffer, the segment counts in their id buffer
    const rtw::RadianceSizes sz = rtw::radiance_sizes(c->precision != RTW_F32, n, n_samples);
    const size_t sums_off = align_up(sz.rays.bytes, 16);
    const size_t rng_off = sums_off + align_up(sz.radiance.bytes, 16);
    rc = ensure(c, &q->d_rays, &q->rays_cap, rng_off + (rng ? sz.rng.bytes : 0));
    if (!rc && colours) rc = ensure(c, &q->d_out, &q->out_cap, sz.colours.bytes);
    if (!rc && segments) rc = ensure(c, &q->d_ids, &q->ids_cap, sz.segments.bytes);
    if (rc) return rc;
    char* base = static_cast<char*>(q->d_rays);
    double* d_sums = reinterpret_cast<double*>(base + sums_off);
    uint64_t* d_rng = rng ? reinterpret_cast<uint64_t*>(base + rng_off) : nullptr;
    HIP_TRY(c, hipMemcpyAsync(q->d_rays, rays, sz.rays.bytes, hipMemcpyHostToDevice, c->stream));
    if (accumulate) HIP_TRY(c, hipMemcpyAsync(d_sums, radiance, sz.radiance.bytes, hipMemcpyHostToDevice, c->stream));
    if (rng) HIP_TRY(c, hipMemcpyAsync(d_rng, rng, sz.rng.bytes, hipMemcpyHostToDevice, c->stream));
    const RadianceCall call{q->d_rays, n, seed, first_stream, first_sample, n_samples, max_depth, background,
                            d_rng, accumulate, d_sums, colours ? q->d_out : nullptr,
                            segments ? static_cast<uint32_t*>(q->d_ids) : nullptr};
    rc = by_precision(c, [&](auto r) { return radiance_device_t<decltype(r)>(c, call, c->stream); });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(radiance, d_sums, sz.radiance.bytes, hipMemcpyDeviceToHost, c->stream));
    if (rng) HIP_TRY(c, hipMemcpyAsync(rng, d_rng, sz.rng.bytes, hipMemcpyDeviceToHost, c->stream));
    if (colours) HIP_TRY(c, hipMemcpyAsync(colours, q->d_out, sz.colours.bytes, hipMemcpyDeviceToHost, c->stream));
    if (segments)
        HIP_TRY(c, hipMemcpyAsync(segments, q->d_ids, sz.segments.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
