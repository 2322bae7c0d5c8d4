// capi_features.cpp -- the feature pass of the C-ABI (include/rtw.h):
// rtw_render_features and its device form.  A pass is plan (host/query_plan.hpp,
// with the camera's center) -> params (feature_params) -> launch -> bookkeeping,
// on the query state's counters and events and its own staging buffers: nothing
// of the render's or of a ray query's is touched.
#include <string>

#include "capi_ctx.hpp"
#include "features_kernels.h"
#include "host/query_plan.hpp"

namespace {

// what both forms refuse before any device call; RTW_OK: the pass can run
int features_checks(rtw_ctx* c, const rtw_camera* cam, uint32_t first, uint32_t n, const double* features) {
    if (!cam) return fail(c, RTW_E_INVALID, "cam is NULL");
    if (!features) return fail(c, RTW_E_INVALID, "features is NULL");
    if (cam->image_width > 65535 || cam->image_height > 65535)
        return fail(c, RTW_E_INVALID, "image width or height beyond 65535");
    if ((uint64_t)first + n > 0xFFFFFFFFull) return fail(c, RTW_E_INVALID, "first_sample + n_samples overflows");
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "the feature pass runs on a one-device context");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    return RTW_OK;
}

template <typename R>
int features_device_t(rtw_ctx* c, const rtw_camera& cam, uint64_t seed, uint32_t first, uint32_t n,
                      const uint32_t* d_counts, double* d_features, int32_t* d_ids, hipStream_t stream) {
    const rtw::DevScene<R>& sc = dev_scene<R>(c);
    const rtw::QueryPlan pl = rtw::plan_query<R>(c->knobs, sc, c->scale, cam.center);
    if (pl.err) return fail(c, pl.err, pl.err_text);
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::FParams<R> p = rtw::feature_params<R>(sc, cam, seed, first, n, pl);
    p.counts = d_counts;
    p.features = d_features;
    p.ids = first == 0 ? d_ids : nullptr;   // sample 0 is traced by a call that starts there
    p.counters = q->d_counters;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, (rtw::kQueryCounters + 1) * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    const int ran = rtw::launch_primary_features(p, pl.world, pl.robust != 0, pl.hit_lds, c->knobs.query_grid, stream);
    if (ran >= 0 && ran != pl.world) return fail(c, RTW_E_DEVICE, "the launched feature kernel is not the plan's");
    if (ran < 0)
        return fail(c, RTW_E_DEVICE,
                    std::string("feature kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.kernel = (uint32_t)ran;
    q->last.is_light_pdf = 0u;
    q->any = true;
    return RTW_OK;
}

}  // namespace

extern "C" {

int rtw_render_features_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample,
                               uint32_t n_samples, const uint32_t* d_counts, size_t counts_bytes, double* d_features,
                               size_t features_bytes, int32_t* d_ids, size_t ids_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = features_checks(c, cam, first_sample, n_samples, d_features);
    if (rc) return rc;
    const size_t px = (size_t)cam->image_width * cam->image_height;
    if (features_bytes < px * rtw::kFeatureChannels * sizeof(double))
        return fail(c, RTW_E_INVALID, "d_features is smaller than H x W x 8 doubles");
    if (reinterpret_cast<uintptr_t>(d_features) % 16) return fail(c, RTW_E_INVALID, "d_features is not 16-byte aligned");
    if (d_counts && counts_bytes < px * sizeof(uint32_t))
        return fail(c, RTW_E_INVALID, "d_counts is smaller than H x W uint32");
    if (d_ids && ids_bytes < px * 2 * sizeof(int32_t)) return fail(c, RTW_E_INVALID, "d_ids is smaller than H x W x 2 int32");
    if (n_samples == 0 || px == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) {
        return features_device_t<decltype(r)>(c, *cam, seed, first_sample, n_samples, d_counts, d_features, d_ids, s);
    });
}

int rtw_render_features(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
                        const uint32_t* counts, double* features, int32_t* ids) {
    if (!c) return RTW_E_INVALID;
    int rc = features_checks(c, cam, first_sample, n_samples, features);
    if (rc) return rc;
    const size_t px = (size_t)cam->image_width * cam->image_height;
    if (n_samples == 0 || px == 0) return RTW_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    const size_t feat_bytes = px * rtw::kFeatureChannels * sizeof(double);
    const size_t counts_bytes = px * sizeof(uint32_t), ids_bytes = px * 2 * sizeof(int32_t);
    // ids are written by a call that starts at sample 0, for the pixels that take a
    // sample: the caller's values go in first, so that the others come back as they were
    const bool with_ids = ids && first_sample == 0;
    rc = ensure(c, &q->d_feat, &q->feat_cap, feat_bytes);
    if (!rc && counts) rc = ensure(c, &q->d_feat_counts, &q->feat_counts_cap, counts_bytes);
    if (!rc && with_ids) rc = ensure(c, &q->d_feat_ids, &q->feat_ids_cap, ids_bytes);
    if (rc) return rc;
    if (first_sample) HIP_TRY(c, hipMemcpyAsync(q->d_feat, features, feat_bytes, hipMemcpyHostToDevice, c->stream));
    if (counts) HIP_TRY(c, hipMemcpyAsync(q->d_feat_counts, counts, counts_bytes, hipMemcpyHostToDevice, c->stream));
    if (with_ids) HIP_TRY(c, hipMemcpyAsync(q->d_feat_ids, ids, ids_bytes, hipMemcpyHostToDevice, c->stream));
    rc = by_precision(c, [&](auto r) {
        return features_device_t<decltype(r)>(c, *cam, seed, first_sample, n_samples,
                                              counts ? reinterpret_cast<const uint32_t*>(q->d_feat_counts) : nullptr,
                                              reinterpret_cast<double*>(q->d_feat),
                                              with_ids ? reinterpret_cast<int32_t*>(q->d_feat_ids) : nullptr, c->stream);
    });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(features, q->d_feat, feat_bytes, hipMemcpyDeviceToHost, c->stream));
    if (with_ids) HIP_TRY(c, hipMemcpyAsync(ids, q->d_feat_ids, ids_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
