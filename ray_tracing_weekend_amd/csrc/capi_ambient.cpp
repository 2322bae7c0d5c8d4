// capi_ambient.cpp -- ambient occlusion as one query of the C-ABI (include/rtw.h):
// rtw_ambient_occlusion and its device form.  As the other queries
// (capi_nee.cpp, capi_direct.cpp): checks (host/ambient_plan.hpp) -> plan
// (host/query_plan.hpp, the closest hit's) -> params -> launch -> bookkeeping,
// on the query state's counters, events and staging buffers.
#include <string>

#include "ambient_kernels.h"
#include "capi_ctx.hpp"
#include "host/ambient_plan.hpp"

namespace {

// what every query refuses before anything else (capi_query.cpp query_checks), then
// the arguments (host/ambient_plan.hpp)
int ambient_checks(rtw_ctx* c, const rtw::AmbientArgs& a) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    const char* text = "";
    const int rc = rtw::ambient_check(a, c->precision != RTW_F32, &text);
    return rc ? fail(c, rc, text) : RTW_OK;
}

struct AmbientCall {
    const void* points;
    uint64_t n, seed, first_stream;
    uint32_t first_sample, n_samples;
    double t_min, t_max;
    int accumulate;
    uint32_t* open;
    void* directions;
    uint8_t* occluded;
};

template <typename R>
int ambient_device_t(rtw_ctx* c, const AmbientCall& a, hipStream_t stream) {
    const rtw::DevScene<R>& sc = dev_scene<R>(c);
    const rtw::QueryPlan pl = rtw::plan_query<R>(c->knobs, sc, c->scale);
    if (pl.err) return fail(c, pl.err, pl.err_text);
    const rtw::AmbientPlan ap = rtw::plan_ambient(pl, sizeof(R) == 8);
    if (ap.err) return fail(c, ap.err, ap.err_text);
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::AParams<R> p{};
    p.sc = sc;
    p.sc.robust = pl.robust;
    p.points = reinterpret_cast<const R*>(a.points);
    p.open = a.open;
    p.directions = reinterpret_cast<R*>(a.directions);
    p.occluded = a.occluded;
    p.seed = a.seed;
    p.first_stream = a.first_stream;
    p.first_sample = a.first_sample;
    p.n_samples = a.n_samples;
    p.counters = q->d_counters;
    p.n = a.n;
    p.tmin = (R)a.t_min;
    p.tmax = (R)a.t_max;
    p.stack = pl.stack;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    // the kernel adds to the counts: a call that does not continue them starts from 0
    if (!a.accumulate) HIP_TRY(c, hipMemsetAsync(a.open, 0, a.n * sizeof(uint32_t), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    const int ran = rtw::launch_ambient(p, pl.world, pl.robust != 0, ap.lds, c->knobs.query_grid, stream);
    if (ran >= 0 && ran != pl.world) return fail(c, RTW_E_DEVICE, "the launched query kernel is not the plan's");
    if (ran < 0)
        return fail(c, RTW_E_DEVICE, std::string("query kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.kernel = (uint32_t)ran;
    q->last.is_light_pdf = rtw::kQueryAmbient;
    q->any = true;
    return RTW_OK;
}

}  // namespace

extern "C" {

int rtw_ambient_occlusion_device(rtw_ctx* c, const void* d_points, size_t points_bytes, uint64_t n, uint64_t seed,
                                 uint64_t first_stream, uint32_t first_sample, uint32_t n_samples, double t_min,
                                 double t_max, int accumulate, uint32_t* d_open, size_t open_bytes,
                                 void* d_directions, size_t directions_bytes, uint8_t* d_occluded,
                                 size_t occluded_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    rtw::AmbientArgs a;
    a.points = d_points, a.n = n, a.n_samples = n_samples, a.t_min = t_min;
    a.open = d_open, a.directions = d_directions, a.occluded = d_occluded;
    a.device = true;
    a.points_bytes = points_bytes, a.open_bytes = open_bytes;
    a.directions_bytes = directions_bytes, a.occluded_bytes = occluded_bytes;
    int rc = ambient_checks(c, a);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const AmbientCall call{d_points, n, seed, first_stream, first_sample, n_samples, t_min, t_max, accumulate,
                           d_open, d_directions, d_occluded};
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) { return ambient_device_t<decltype(r)>(c, call, s); });
}

int rtw_ambient_occlusion(rtw_ctx* c, const void* points, uint64_t n, uint64_t seed, uint64_t first_stream,
                          uint32_t first_sample, uint32_t n_samples, double t_min, double t_max, int accumulate,
                          uint32_t* open, void* directions, uint8_t* occluded) {
    if (!c) return RTW_E_INVALID;
    rtw::AmbientArgs a;
    a.points = points, a.n = n, a.n_samples = n_samples, a.t_min = t_min;
    a.open = open, a.directions = directions, a.occluded = occluded;
    int rc = ambient_checks(c, a);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: points | counts in the queries' ray buffer (the counts from the next 16-byte
    // boundary), the directions in their record buffer, the bytes in their id buffer
    const rtw::AmbientSizes sz = rtw::ambient_sizes(c->precision != RTW_F32, n, n_samples);
    const size_t open_off = (sz.points.bytes + 15u) & ~(size_t)15u;
    rc = ensure(c, &q->d_rays, &q->rays_cap, open_off + sz.open.bytes);
    if (!rc && directions) rc = ensure(c, &q->d_out, &q->out_cap, sz.directions.bytes);
    if (!rc && occluded) rc = ensure(c, &q->d_ids, &q->ids_cap, sz.occluded.bytes);
    if (rc) return rc;
    uint32_t* d_open = reinterpret_cast<uint32_t*>(static_cast<char*>(q->d_rays) + open_off);
    HIP_TRY(c, hipMemcpyAsync(q->d_rays, points, sz.points.bytes, hipMemcpyHostToDevice, c->stream));
    if (accumulate) HIP_TRY(c, hipMemcpyAsync(d_open, open, sz.open.bytes, hipMemcpyHostToDevice, c->stream));
    const AmbientCall call{q->d_rays, n, seed, first_stream, first_sample, n_samples, t_min, t_max, accumulate,
                           d_open, directions ? q->d_out : nullptr,
                           occluded ? static_cast<uint8_t*>(q->d_ids) : nullptr};
    rc = by_precision(c, [&](auto r) { return ambient_device_t<decltype(r)>(c, call, c->stream); });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(open, d_open, sz.open.bytes, hipMemcpyDeviceToHost, c->stream));
    if (directions)
        HIP_TRY(c, hipMemcpyAsync(directions, q->d_out, sz.directions.bytes, hipMemcpyDeviceToHost, c->stream));
    if (occluded)
        HIP_TRY(c, hipMemcpyAsync(occluded, q->d_ids, sz.occluded.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
