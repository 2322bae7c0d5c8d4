// capi_direct.cpp -- direct lighting as one query of the C-ABI (include/rtw.h):
// rtw_direct_light and its device form.  As the other queries (capi_query.cpp,
// capi_nee.cpp): checks (host/direct_plan.hpp) -> plan (host/query_plan.hpp, the
// closest hit's and the light pdf's) -> params -> launch -> bookkeeping, on the
// query state's counters, events and staging buffers.
#include <string>

#include "capi_ctx.hpp"
#include "direct_kernels.h"
#include "host/direct_plan.hpp"

namespace {

// what every query refuses before anything else (capi_query.cpp query_checks), then
// the arguments (host/direct_plan.hpp)
int direct_checks(rtw_ctx* c, const rtw::DirectArgs& a) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    const bool f64 = c->precision != RTW_F32;
    const char* text = "";
    const int rc = rtw::direct_check(a, f64, f64 ? c->sc64.n_list : c->sc32.n_list, &text);
    return rc ? fail(c, rc, text) : RTW_OK;
}

struct DirectCall {
    const void* points;
    uint64_t n, seed, first_stream;
    uint32_t first_sample, n_samples;
    double t_min;
    int accumulate;
    double* direct;
    void* samples;
    int32_t* sample_ids;
};

template <typename R>
int direct_device_t(rtw_ctx* c, const DirectCall& a, hipStream_t stream) {
    const rtw::DevScene<R>& sc = dev_scene<R>(c);
    const rtw::QueryPlan pl = rtw::plan_query<R>(c->knobs, sc, c->scale);
    if (pl.err) return fail(c, pl.err, pl.err_text);
    const rtw::DirectPlan dp = rtw::plan_direct(pl, sizeof(R) == 8);
    if (dp.err) return fail(c, dp.err, dp.err_text);
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::DParams<R> p{};
    p.sc = sc;
    p.sc.robust = pl.robust;
    p.points = reinterpret_cast<const R*>(a.points);
    p.direct = a.direct;
    p.samples = reinterpret_cast<R*>(a.samples);
    p.sample_ids = a.sample_ids;
    p.seed = a.seed;
    p.first_stream = a.first_stream;
    p.first_sample = a.first_sample;
    p.n_samples = a.n_samples;
    p.accumulate = a.accumulate ? 1u : 0u;
    p.light_path = pl.light_path;
    p.counters = q->d_counters;
    p.n = a.n;
    p.tmin = (R)a.t_min;
    p.stack = pl.stack;
    p.light_stack = pl.light_stack;
    p.light_off = dp.light_off;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    const int ran = rtw::launch_direct_light(p, pl.world, pl.robust != 0, dp.lds, c->knobs.query_grid, stream);
    if (ran >= 0 && ran != pl.world) return fail(c, RTW_E_DEVICE, "the launched query kernel is not the plan's");
    if (ran < 0)
        return fail(c, RTW_E_DEVICE, std::string("query kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.kernel = (uint32_t)ran;
    q->last.is_light_pdf = rtw::kQueryDirectLight;
    q->any = true;
    return RTW_OK;
}

}  // namespace

extern "C" {

int rtw_direct_light_device(rtw_ctx* c, const void* d_points, size_t points_bytes, uint64_t n, uint64_t seed,
                            uint64_t first_stream, uint32_t first_sample, uint32_t n_samples, double t_min,
                            int accumulate, double* d_direct, size_t direct_bytes, void* d_samples,
                            size_t samples_bytes, int32_t* d_sample_ids, size_t sample_ids_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    rtw::DirectArgs a;
    a.points = d_points, a.n = n, a.n_samples = n_samples, a.t_min = t_min;
    a.direct = d_direct, a.samples = d_samples, a.sample_ids = d_sample_ids;
    a.device = true;
    a.points_bytes = points_bytes, a.direct_bytes = direct_bytes;
    a.samples_bytes = samples_bytes, a.sample_ids_bytes = sample_ids_bytes;
    int rc = direct_checks(c, a);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const DirectCall call{d_points, n, seed, first_stream, first_sample, n_samples, t_min, accumulate,
                          d_direct, d_samples, d_sample_ids};
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) { return direct_device_t<decltype(r)>(c, call, s); });
}

int rtw_direct_light(rtw_ctx* c, const void* points, uint64_t n, uint64_t seed, uint64_t first_stream,
                     uint32_t first_sample, uint32_t n_samples, double t_min, int accumulate, double* direct,
                     void* samples, int32_t* sample_ids) {
    if (!c) return RTW_E_INVALID;
    rtw::DirectArgs a;
    a.points = points, a.n = n, a.n_samples = n_samples, a.t_min = t_min;
    a.direct = direct, a.samples = samples, a.sample_ids = sample_ids;
    int rc = direct_checks(c, a);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: points | sums in the queries' ray buffer (the sums from the next 16-byte
    // boundary), the sample records in their record buffer, the ids in their id buffer
    const rtw::DirectSizes sz = rtw::direct_sizes(c->precision != RTW_F32, n, n_samples);
    const size_t sums_off = (sz.points.bytes + 15u) & ~(size_t)15u;
    rc = ensure(c, &q->d_rays, &q->rays_cap, sums_off + sz.direct.bytes);
    if (!rc && samples) rc = ensure(c, &q->d_out, &q->out_cap, sz.samples.bytes);
    if (!rc && sample_ids) rc = ensure(c, &q->d_ids, &q->ids_cap, sz.sample_ids.bytes);
    if (rc) return rc;
    double* d_sums = reinterpret_cast<double*>(static_cast<char*>(q->d_rays) + sums_off);
    HIP_TRY(c, hipMemcpyAsync(q->d_rays, points, sz.points.bytes, hipMemcpyHostToDevice, c->stream));
    // (a skipped point's row is not written: the caller's content goes there and back)
    HIP_TRY(c, hipMemcpyAsync(d_sums, direct, sz.direct.bytes, hipMemcpyHostToDevice, c->stream));
    const DirectCall call{q->d_rays, n, seed, first_stream, first_sample, n_samples, t_min, accumulate,
                          d_sums, samples ? q->d_out : nullptr,
                          sample_ids ? static_cast<int32_t*>(q->d_ids) : nullptr};
    rc = by_precision(c, [&](auto r) { return direct_device_t<decltype(r)>(c, call, c->stream); });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(direct, d_sums, sz.direct.bytes, hipMemcpyDeviceToHost, c->stream));
    if (samples) HIP_TRY(c, hipMemcpyAsync(samples, q->d_out, sz.samples.bytes, hipMemcpyDeviceToHost, c->stream));
    if (sample_ids)
        HIP_TRY(c, hipMemcpyAsync(sample_ids, q->d_ids, sz.sample_ids.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
