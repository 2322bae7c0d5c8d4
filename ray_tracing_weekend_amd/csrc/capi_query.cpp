// capi_query.cpp -- the batched ray queries of the C-ABI (include/rtw.h):
// rtw_hit_rays / rtw_light_pdf_rays, their device forms and rtw_get_query_stats.
// A query is plan (host/query_plan.hpp) -> params -> launch -> bookkeeping, on
// its own buffers, counters and events: the render's caches (task order, split,
// windows, stats) are not touched.
#include <cmath>
#include <new>
#include <string>

#include "capi_ctx.hpp"
#include "host/query_plan.hpp"
#include "wavefront_kernels.h"

void destroy_query(rtw_ctx* c) {
    QueryState* q = c->query;
    if (!q) return;
    if (q->d_counters) (void)hipFree(q->d_counters);
    if (q->d_rays) (void)hipFree(q->d_rays);
    if (q->d_out) (void)hipFree(q->d_out);
    if (q->d_ids) (void)hipFree(q->d_ids);
    if (q->d_feat) (void)hipFree(q->d_feat);
    if (q->d_feat_counts) (void)hipFree(q->d_feat_counts);
    if (q->d_feat_ids) (void)hipFree(q->d_feat_ids);
    if (q->d_wf) (void)hipFree(q->d_wf);
    if (q->d_wf_sums) (void)hipFree(q->d_wf_sums);
    if (q->d_wf_words) (void)hipFree(q->d_wf_words);
    if (q->h_wf_count) (void)hipHostFree(q->h_wf_count);
    if (q->ev_span) (void)hipEventDestroy(q->ev_span);
    if (q->ev0) (void)hipEventDestroy(q->ev0);
    if (q->ev1) (void)hipEventDestroy(q->ev1);
    delete q;
    c->query = nullptr;
}

int query_state(rtw_ctx* c) {
    if (c->query) return RTW_OK;
    QueryState* q = new (std::nothrow) QueryState();
    if (!q) return fail(c, RTW_E_DEVICE, "out of memory");
    c->query = q;
    // (one more word than the queries count in: the feature pass's tile counter)
    HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&q->d_counters),
                         (rtw::kQueryCounters + 1) * sizeof(unsigned long long)));
    HIP_TRY(c, hipEventCreate(&q->ev0));
    HIP_TRY(c, hipEventCreate(&q->ev1));
    return RTW_OK;
}

namespace {

// what both queries refuse before anything else; RTW_OK: the context can run one
int query_checks(rtw_ctx* c, const void* rays, uint64_t n) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (n && !rays) return fail(c, RTW_E_INVALID, "rays is NULL");
    if (n > (uint64_t)1 << 40) return fail(c, RTW_E_INVALID, "more than 2^40 rays in one query");
    return RTW_OK;
}

enum QueryKind { kHit, kLightPdf };

template <typename R>
int query_device_t(rtw_ctx* c, QueryKind kind, const void* d_rays, uint64_t n, double t_min, void* d_out,
                   int32_t* d_ids, hipStream_t stream) {
    const rtw::DevScene<R>& sc = dev_scene<R>(c);
    const rtw::QueryPlan pl = rtw::plan_query<R>(c->knobs, sc, c->scale);
    if (pl.err) return fail(c, pl.err, pl.err_text);
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::QParams<R> p{};
    p.sc = sc;
    p.sc.robust = pl.robust;
    p.rays = reinterpret_cast<const R*>(d_rays);
    p.counters = q->d_counters;
    p.n = n;
    p.tmin = (R)t_min;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    int ran;
    if (kind == kHit) {
        p.hits = reinterpret_cast<R*>(d_out);
        p.ids = d_ids;
        p.stack = pl.stack;
        ran = rtw::launch_hit_rays(p, pl.world, pl.robust != 0, pl.hit_lds, c->knobs.query_grid, stream);
        if (ran >= 0 && ran != pl.world) return fail(c, RTW_E_DEVICE, "the launched query kernel is not the plan's");
    } else {
        p.pdf = reinterpret_cast<R*>(d_out);
        p.stack = pl.light_stack;
        ran = rtw::launch_light_pdf_rays(p, pl.light_path, pl.robust != 0, pl.light_lds, c->knobs.query_grid, stream);
        if (ran >= 0 && ran != pl.light_path) return fail(c, RTW_E_DEVICE, "the launched query kernel is not the plan's");
    }
    if (ran < 0)
        return fail(c, RTW_E_DEVICE, std::string("query kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.kernel = (uint32_t)ran;
    q->last.is_light_pdf = kind == kLightPdf ? 1u : 0u;
    q->any = true;
    return RTW_OK;
}

// the host forms: stage the rays, run the device form on the context's stream, read back
int query_host(rtw_ctx* c, QueryKind kind, const void* rays, uint64_t n, double t_min, void* out, int32_t* ids) {
    const size_t esz = c->precision == RTW_F32 ? sizeof(float) : sizeof(double);
    const size_t out_per = kind == kHit ? 9 * esz : esz;
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rc = ensure(c, &q->d_rays, &q->rays_cap, n * 6 * esz);
    if (!rc) rc = ensure(c, &q->d_out, &q->out_cap, n * out_per);
    if (!rc && kind == kHit) rc = ensure(c, &q->d_ids, &q->ids_cap, n * 4 * sizeof(int32_t));
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(q->d_rays, rays, n * 6 * esz, hipMemcpyHostToDevice, c->stream));
    rc = by_precision(c, [&](auto r) {
        return query_device_t<decltype(r)>(c, kind, q->d_rays, n, t_min, q->d_out, reinterpret_cast<int32_t*>(q->d_ids),
                                           c->stream);
    });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the upload reads `rays`)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(out, q->d_out, n * out_per, hipMemcpyDeviceToHost, c->stream));
    if (kind == kHit) HIP_TRY(c, hipMemcpyAsync(ids, q->d_ids, n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

bool bad_t_min(double t_min) { return !(t_min >= 0.0) || !std::isfinite(t_min); }

}  // namespace

extern "C" {

int rtw_hit_rays_device(rtw_ctx* c, const void* d_rays, uint64_t n, double t_min, void* d_hits, size_t hits_bytes,
                        int32_t* d_ids, size_t ids_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = query_checks(c, d_rays, n);
    if (rc) return rc;
    if (bad_t_min(t_min)) return fail(c, RTW_E_INVALID, "t_min must be finite and >= 0");
    if (n == 0) return RTW_OK;
    const size_t esz = c->precision == RTW_F32 ? sizeof(float) : sizeof(double);
    if (!d_hits || !d_ids) return fail(c, RTW_E_INVALID, "d_hits or d_ids is NULL");
    if (hits_bytes < n * 9 * esz) return fail(c, RTW_E_INVALID, "d_hits is smaller than n x 9 values");
    if (ids_bytes < n * 4 * sizeof(int32_t)) return fail(c, RTW_E_INVALID, "d_ids is smaller than n x 4 int32");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) {
        return query_device_t<decltype(r)>(c, kHit, d_rays, n, t_min, d_hits, d_ids, s);
    });
}

int rtw_hit_rays(rtw_ctx* c, const void* rays, uint64_t n, double t_min, void* hits, int32_t* ids) {
    if (!c) return RTW_E_INVALID;
    int rc = query_checks(c, rays, n);
    if (rc) return rc;
    if (bad_t_min(t_min)) return fail(c, RTW_E_INVALID, "t_min must be finite and >= 0");
    if (n == 0) return RTW_OK;
    if (!hits || !ids) return fail(c, RTW_E_INVALID, "hits or ids is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    return query_host(c, kHit, rays, n, t_min, hits, ids);
}

int rtw_light_pdf_rays_device(rtw_ctx* c, const void* d_rays, uint64_t n, void* d_pdf, size_t pdf_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = query_checks(c, d_rays, n);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    const size_t esz = c->precision == RTW_F32 ? sizeof(float) : sizeof(double);
    if (!d_pdf) return fail(c, RTW_E_INVALID, "d_pdf is NULL");
    if (pdf_bytes < n * esz) return fail(c, RTW_E_INVALID, "d_pdf is smaller than n values");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) {
        return query_device_t<decltype(r)>(c, kLightPdf, d_rays, n, 0.0, d_pdf, nullptr, s);
    });
}

int rtw_light_pdf_rays(rtw_ctx* c, const void* rays, uint64_t n, void* pdf) {
    if (!c) return RTW_E_INVALID;
    int rc = query_checks(c, rays, n);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    if (!pdf) return fail(c, RTW_E_INVALID, "pdf is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    return query_host(c, kLightPdf, rays, n, 0.0, pdf, nullptr);
}

int rtw_get_query_stats(rtw_ctx* c, rtw_query_stats* out) {
    if (!c || !out) return fail(c, RTW_E_INVALID, "bad argument");
    QueryState* q = c->query;
    if (!q || !q->any) return fail(c, RTW_E_INVALID, "no query yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(q->ev1));
    unsigned long long h[rtw::kQueryCounters] = {};
    HIP_TRY(c, hipMemcpy(h, q->d_counters, sizeof h, hipMemcpyDeviceToHost));
    float ms = 0.f;
    // (a driver call spans many queries, each with its own ev0: it starts at ev_span)
    const bool span = q->last.is_light_pdf == rtw::kQueryWavefront && q->ev_span;
    HIP_TRY(c, hipEventElapsedTime(&ms, span ? q->ev_span : q->ev0, q->ev1));
    q->last.rays = h[rtw::kQcRays];
    q->last.hits = h[rtw::kQcHits];
    q->last.node_visits = h[rtw::kQcNodeVisits];
    q->last.sphere_tests = h[rtw::kQcSphereTests];
    q->last.light_tests = h[rtw::kQcLightTests];
    q->last.kernel_ms = ms;
    *out = q->last;
    return RTW_OK;
}

}  // extern "C"
