// capi_nee.cpp -- the any-hit and light-sampling queries of the C-ABI
// (include/rtw.h): rtw_occluded_rays / rtw_light_sample and their device forms.
// As the other queries (capi_query.cpp): plan (host/query_plan.hpp, the closest
// hit's and the light pdf's) -> params -> launch -> bookkeeping, on the query
// state's counters, events and staging buffers.
#include <cmath>
#include <string>

#include "capi_ctx.hpp"
#include "host/query_plan.hpp"
#include "nee_kernels.h"

namespace {

// what every query refuses before anything else (capi_query.cpp query_checks)
int nee_checks(rtw_ctx* c, const void* in, uint64_t n, const char* what) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (n && !in) return fail(c, RTW_E_INVALID, std::string(what) + " is NULL");
    if (n > (uint64_t)1 << 40) return fail(c, RTW_E_INVALID, "more than 2^40 rays in one query");
    return RTW_OK;
}

bool bad_t_min(double t_min) { return !(t_min >= 0.0) || !std::isfinite(t_min); }

size_t elem(const rtw_ctx* c) { return c->precision == RTW_F32 ? sizeof(float) : sizeof(double); }

// HittableList::random indexes gen_range(0..len) and panics on an empty list
// (hittable_list.rs:417)
int empty_list_check(rtw_ctx* c) {
    const uint32_t n_list = c->precision == RTW_F32 ? c->sc32.n_list : c->sc64.n_list;
    if (n_list == 0)
        return fail(c, RTW_E_INVALID, "rtw_light_sample: the light list is empty (the reference panics, "
                                      "hittable_list.rs:417)");
    return RTW_OK;
}

struct NeeArgs {
    bool sample;                       // rtw_light_sample, else rtw_occluded_rays
    const void* in;                    // rays n x 6 / origins n x 3
    const void* t_max;
    double t_min;
    uint8_t* occluded;
    uint64_t seed, first_stream;
    uint32_t sample_index;
    void* dirs;
    void* pdf;
    int32_t* light;
};

template <typename R>
int nee_device_t(rtw_ctx* c, const NeeArgs& a, uint64_t n, hipStream_t stream) {
    const rtw::DevScene<R>& sc = dev_scene<R>(c);
    const rtw::QueryPlan pl = rtw::plan_query<R>(c->knobs, sc, c->scale);
    if (pl.err) return fail(c, pl.err, pl.err_text);
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::NParams<R> p{};
    p.sc = sc;
    p.sc.robust = pl.robust;
    p.counters = q->d_counters;
    p.n = n;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    int ran, want;
    if (!a.sample) {
        p.rays = reinterpret_cast<const R*>(a.in);
        p.tmax = reinterpret_cast<const R*>(a.t_max);
        p.occluded = a.occluded;
        p.tmin = (R)a.t_min;
        p.stack = pl.stack;
        want = pl.world;
        ran = rtw::launch_occlusion(p, pl.world, pl.robust != 0, pl.hit_lds, c->knobs.query_grid, stream);
    } else {
        p.origins = reinterpret_cast<const R*>(a.in);
        p.dirs = reinterpret_cast<R*>(a.dirs);
        p.pdf = reinterpret_cast<R*>(a.pdf);
        p.light = a.light;
        p.seed = a.seed;
        p.first_stream = a.first_stream;
        p.sample = a.sample_index;
        p.stack = pl.light_stack;
        want = pl.light_path;
        ran = rtw::launch_light_sample(p, pl.light_path, pl.robust != 0, pl.light_lds, c->knobs.query_grid, stream);
    }
    if (ran >= 0 && ran != want) return fail(c, RTW_E_DEVICE, "the launched query kernel is not the plan's");
    if (ran < 0)
        return fail(c, RTW_E_DEVICE, std::string("query kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.kernel = (uint32_t)ran;
    q->last.is_light_pdf = a.sample ? rtw::kQueryLightSample : rtw::kQueryAnyHit;
    q->any = true;
    return RTW_OK;
}

int nee_device(rtw_ctx* c, const NeeArgs& a, uint64_t n, hipStream_t stream) {
    return by_precision(c, [&](auto r) { return nee_device_t<decltype(r)>(c, a, n, stream); });
}

}  // namespace

extern "C" {

int rtw_occluded_rays_device(rtw_ctx* c, const void* d_rays, uint64_t n, double t_min, const void* d_t_max,
                             size_t t_max_bytes, uint8_t* d_occluded, size_t occluded_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = nee_checks(c, d_rays, n, "d_rays");
    if (rc) return rc;
    if (bad_t_min(t_min)) return fail(c, RTW_E_INVALID, "t_min must be finite and >= 0");
    if (n == 0) return RTW_OK;
    if (!d_occluded) return fail(c, RTW_E_INVALID, "d_occluded is NULL");
    if (d_t_max && t_max_bytes < n * elem(c)) return fail(c, RTW_E_INVALID, "d_t_max is smaller than n values");
    if (occluded_bytes < n) return fail(c, RTW_E_INVALID, "d_occluded is smaller than n bytes");
    HIP_TRY(c, hipSetDevice(c->device));
    NeeArgs a{};
    a.in = d_rays;
    a.t_max = d_t_max;
    a.t_min = t_min;
    a.occluded = d_occluded;
    return nee_device(c, a, n, resolve_stream(c, stream));
}

int rtw_occluded_rays(rtw_ctx* c, const void* rays, uint64_t n, double t_min, const void* t_max, uint8_t* occluded) {
    if (!c) return RTW_E_INVALID;
    int rc = nee_checks(c, rays, n, "rays");
    if (rc) return rc;
    if (bad_t_min(t_min)) return fail(c, RTW_E_INVALID, "t_min must be finite and >= 0");
    if (n == 0) return RTW_OK;
    if (!occluded) return fail(c, RTW_E_INVALID, "occluded is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: rays | t_max in the queries' ray buffer, the bytes in their record buffer
    const size_t esz = elem(c), rays_b = n * 6 * esz;
    rc = ensure(c, &q->d_rays, &q->rays_cap, rays_b + n * esz);
    if (!rc) rc = ensure(c, &q->d_out, &q->out_cap, n);
    if (rc) return rc;
    char* d_tmax = t_max ? static_cast<char*>(q->d_rays) + rays_b : nullptr;
    HIP_TRY(c, hipMemcpyAsync(q->d_rays, rays, rays_b, hipMemcpyHostToDevice, c->stream));
    if (t_max) HIP_TRY(c, hipMemcpyAsync(d_tmax, t_max, n * esz, hipMemcpyHostToDevice, c->stream));
    NeeArgs a{};
    a.in = q->d_rays;
    a.t_max = d_tmax;
    a.t_min = t_min;
    a.occluded = static_cast<uint8_t*>(q->d_out);
    rc = nee_device(c, a, n, c->stream);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(occluded, q->d_out, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

int rtw_light_sample_device(rtw_ctx* c, const void* d_origins, uint64_t n, uint64_t seed, uint64_t first_stream,
                            uint32_t sample, void* d_directions, size_t directions_bytes, void* d_pdf,
                            size_t pdf_bytes, int32_t* d_light, size_t light_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = nee_checks(c, d_origins, n, "d_origins");
    if (rc) return rc;
    rc = empty_list_check(c);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    if (!d_directions) return fail(c, RTW_E_INVALID, "d_directions is NULL");
    if (directions_bytes < n * 3 * elem(c)) return fail(c, RTW_E_INVALID, "d_directions is smaller than n x 3 values");
    if (d_pdf && pdf_bytes < n * elem(c)) return fail(c, RTW_E_INVALID, "d_pdf is smaller than n values");
    if (d_light && light_bytes < n * sizeof(int32_t)) return fail(c, RTW_E_INVALID, "d_light is smaller than n int32");
    HIP_TRY(c, hipSetDevice(c->device));
    NeeArgs a{};
    a.sample = true;
    a.in = d_origins;
    a.seed = seed;
    a.first_stream = first_stream;
    a.sample_index = sample;
    a.dirs = d_directions;
    a.pdf = d_pdf;
    a.light = d_light;
    return nee_device(c, a, n, resolve_stream(c, stream));
}

int rtw_light_sample(rtw_ctx* c, const void* origins, uint64_t n, uint64_t seed, uint64_t first_stream, uint32_t sample,
                     void* directions, void* pdf, int32_t* light) {
    if (!c) return RTW_E_INVALID;
    int rc = nee_checks(c, origins, n, "origins");
    if (rc) return rc;
    rc = empty_list_check(c);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    if (!directions) return fail(c, RTW_E_INVALID, "directions is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: origins in the queries' ray buffer, directions | pdf in their record
    // buffer, the list indices in their id buffer
    const size_t esz = elem(c), dirs_b = n * 3 * esz;
    rc = ensure(c, &q->d_rays, &q->rays_cap, dirs_b);
    if (!rc) rc = ensure(c, &q->d_out, &q->out_cap, dirs_b + n * esz);
    if (!rc && light) rc = ensure(c, &q->d_ids, &q->ids_cap, n * sizeof(int32_t));
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(q->d_rays, origins, dirs_b, hipMemcpyHostToDevice, c->stream));
    NeeArgs a{};
    a.sample = true;
    a.in = q->d_rays;
    a.seed = seed;
    a.first_stream = first_stream;
    a.sample_index = sample;
    a.dirs = q->d_out;
    a.pdf = pdf ? static_cast<char*>(q->d_out) + dirs_b : nullptr;
    a.light = light ? static_cast<int32_t*>(q->d_ids) : nullptr;
    rc = nee_device(c, a, n, c->stream);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the upload reads `origins`)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(directions, q->d_out, dirs_b, hipMemcpyDeviceToHost, c->stream));
    if (pdf) HIP_TRY(c, hipMemcpyAsync(pdf, a.pdf, n * esz, hipMemcpyDeviceToHost, c->stream));
    if (light) HIP_TRY(c, hipMemcpyAsync(light, q->d_ids, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
