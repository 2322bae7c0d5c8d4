// capi_path.cpp -- the two path queries of the C-ABI (include/rtw.h):
// rtw_camera_rays / rtw_shade_rays and their device forms.  As the other queries
// (capi_query.cpp, capi_nee.cpp): plan (host/query_plan.hpp, the light pdf's) ->
// params (host/path_params.hpp) -> launch -> bookkeeping, on the query state's
// counters, events and staging buffers.
#include <string>

#include "capi_ctx.hpp"
#include "host/path_params.hpp"
#include "host/query_plan.hpp"
#include "path_kernels.h"

namespace {

size_t elem(const rtw_ctx* c) { return c->precision == RTW_F32 ? sizeof(float) : sizeof(double); }

// a device buffer of records of `record_bytes` must start where the kernel's widest
// access to such a record is aligned (path_kernels.h record_align); NULL passes
bool misaligned(const void* p, size_t record_bytes) {
    return reinterpret_cast<uintptr_t>(p) % rtw::record_align(record_bytes) != 0;
}

// what both forms of rtw_camera_rays refuse before any device call (no scene is needed)
int camera_checks(rtw_ctx* c, const rtw_camera* cam, uint64_t first_pixel, uint64_t n, bool listed) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    if (!cam) return fail(c, RTW_E_INVALID, "cam is NULL");
    if (n > (uint64_t)1 << 40) return fail(c, RTW_E_INVALID, "more than 2^40 rays in one query");
    const uint64_t px = (uint64_t)cam->image_width * cam->image_height;
    if (!listed && n && (first_pixel >= px || n > px - first_pixel))
        return fail(c, RTW_E_INVALID, "first_pixel + n is beyond the image's W x H pixels");
    if (listed && n && px == 0) return fail(c, RTW_E_INVALID, "the image has no pixels");
    return RTW_OK;
}

// what both forms of rtw_shade_rays refuse before any device call
int shade_checks(rtw_ctx* c, const void* rays, const void* hits, const void* ids, uint64_t n) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (n && (!rays || !hits || !ids)) return fail(c, RTW_E_INVALID, "rays, hits or ids is NULL");
    if (n > (uint64_t)1 << 40) return fail(c, RTW_E_INVALID, "more than 2^40 rays in one query");
    // MixturePdf::generate draws from the light list (hittable_list.rs:417 panics on an
    // empty one); the render carries a NaN on, a bounce query refuses
    const uint32_t n_list = c->precision == RTW_F32 ? c->sc32.n_list : c->sc64.n_list;
    if (n_list == 0 && c->has_lambertian)
        return fail(c, RTW_E_NO_LIGHTS, "rtw_shade_rays: the light list is empty and the scene holds a Lambertian "
                                        "material (the reference panics, hittable_list.rs:417)");
    return RTW_OK;
}

struct ShadeBufs {
    const void* rays;
    const void* hits;
    const int32_t* ids;
    uint64_t* rng;
    void* next;
    void* weight;
    void* emitted;
    int32_t* event;
    void* pdfs;
};

int launched(rtw_ctx* c, int ran, int want, uint32_t kind, hipStream_t stream) {
    QueryState* q = c->query;
    if (ran >= 0 && ran != want) return fail(c, RTW_E_DEVICE, "the launched query kernel is not the plan's");
    if (ran < 0)
        return fail(c, RTW_E_DEVICE, std::string("query kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.kernel = (uint32_t)ran;
    q->last.is_light_pdf = kind;
    q->any = true;
    return RTW_OK;
}

template <typename R>
int camera_device_t(rtw_ctx* c, const rtw_camera& cam, uint64_t seed, uint32_t sample, const uint32_t* d_pixels,
                    uint64_t first_pixel, uint64_t n, void* d_rays, uint64_t* d_rng, hipStream_t stream) {
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::CParams<R> p = rtw::camera_ray_params<R>(cam, seed, sample, first_pixel, n);
    p.pixels = d_pixels;
    p.rays = reinterpret_cast<R*>(d_rays);
    p.rng = d_rng;
    p.counters = q->d_counters;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    return launched(c, rtw::launch_camera_rays(p, rtw::kQueryLdsMin, c->knobs.query_grid, stream), 0, rtw::kQueryCameraRays,
                    stream);
}

template <typename R>
int shade_device_t(rtw_ctx* c, const ShadeBufs& b, uint64_t n, hipStream_t stream) {
    const rtw::DevScene<R>& sc = dev_scene<R>(c);
    const rtw::QueryPlan pl = rtw::plan_query<R>(c->knobs, sc, c->scale);
    if (pl.err) return fail(c, pl.err, pl.err_text);
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rtw::SParams<R> p = rtw::shade_params<R>(sc, pl, n);
    p.rays = reinterpret_cast<const R*>(b.rays);
    p.hits = reinterpret_cast<const R*>(b.hits);
    p.ids = b.ids;
    p.rng = b.rng;
    p.next = reinterpret_cast<R*>(b.next);
    p.weight = reinterpret_cast<R*>(b.weight);
    p.emitted = reinterpret_cast<R*>(b.emitted);
    p.event = b.event;
    p.pdfs = reinterpret_cast<R*>(b.pdfs);
    p.counters = q->d_counters;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    const rtw::ShadeLaunch sl = rtw::shade_launch(pl);
    return launched(c, rtw::launch_shade_rays(p, sl.path, sl.robust, sl.lds, c->knobs.query_grid, stream), sl.path,
                    rtw::kQueryShade, stream);
}

// the host forms' staging: one allocation of 16-byte aligned parts (the queries' record buffer)
struct Parts {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t at = total;
        total += align_up(bytes, 16);
        return at;
    }
};

}  // namespace

extern "C" {

int rtw_camera_rays_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t sample, const uint32_t* d_pixels,
                           size_t pixels_bytes, uint64_t first_pixel, uint64_t n, void* d_rays, size_t rays_bytes,
                           uint64_t* d_rng, size_t rng_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = camera_checks(c, cam, first_pixel, n, d_pixels != nullptr);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    if (!d_rays || !d_rng) return fail(c, RTW_E_INVALID, "d_rays or d_rng is NULL");
    if (d_pixels && pixels_bytes < n * sizeof(uint32_t)) return fail(c, RTW_E_INVALID, "d_pixels is smaller than n uint32");
    if (rays_bytes < n * 6 * elem(c)) return fail(c, RTW_E_INVALID, "d_rays is smaller than n x 6 values");
    if (rng_bytes < n * 4 * sizeof(uint64_t)) return fail(c, RTW_E_INVALID, "d_rng is smaller than n x 4 uint64");
    if (misaligned(d_rays, 6 * elem(c)) || misaligned(d_rng, 32))
        return fail(c, RTW_E_INVALID, "d_rays or d_rng is not aligned for its records (rtw.h)");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    return by_precision(c, [&](auto r) {
        return camera_device_t<decltype(r)>(c, *cam, seed, sample, d_pixels, first_pixel, n, d_rays, d_rng, s);
    });
}

int rtw_camera_rays(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t sample, const uint32_t* pixels,
                    uint64_t first_pixel, uint64_t n, void* rays, uint64_t* rng) {
    if (!c) return RTW_E_INVALID;
    int rc = camera_checks(c, cam, first_pixel, n, pixels != nullptr);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    if (!rays || !rng) return fail(c, RTW_E_INVALID, "rays or rng is NULL");
    const uint64_t px = (uint64_t)cam->image_width * cam->image_height;
    if (pixels)
        for (uint64_t k = 0; k < n; ++k)
            if (pixels[k] >= px) return fail(c, RTW_E_INVALID, "a pixel index is beyond the image's W x H pixels");
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: the pixel list in the queries' ray buffer, rays | rng in their record buffer
    const size_t rays_b = n * 6 * elem(c), rng_b = n * 4 * sizeof(uint64_t);
    Parts out;
    const size_t at_rays = out.add(rays_b), at_rng = out.add(rng_b);
    rc = ensure(c, &q->d_out, &q->out_cap, out.total);
    if (!rc && pixels) rc = ensure(c, &q->d_rays, &q->rays_cap, n * sizeof(uint32_t));
    if (rc) return rc;
    if (pixels) HIP_TRY(c, hipMemcpyAsync(q->d_rays, pixels, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    char* base = static_cast<char*>(q->d_out);
    rc = by_precision(c, [&](auto r) {
        return camera_device_t<decltype(r)>(c, *cam, seed, sample,
                                            pixels ? static_cast<const uint32_t*>(q->d_rays) : nullptr, first_pixel, n,
                                            base + at_rays, reinterpret_cast<uint64_t*>(base + at_rng), c->stream);
    });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the upload reads `pixels`)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(rays, base + at_rays, rays_b, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rng, base + at_rng, rng_b, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

int rtw_shade_rays_device(rtw_ctx* c, const void* d_rays, size_t rays_bytes, const void* d_hits, size_t hits_bytes,
                          const int32_t* d_ids, size_t ids_bytes, uint64_t n, uint64_t* d_rng, size_t rng_bytes,
                          void* d_next, size_t next_bytes, void* d_weight, size_t weight_bytes, void* d_emitted,
                          size_t emitted_bytes, int32_t* d_event, size_t event_bytes, void* d_pdfs, size_t pdfs_bytes,
                          void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = shade_checks(c, d_rays, d_hits, d_ids, n);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    if (!d_rng || !d_next || !d_weight || !d_emitted || !d_event)
        return fail(c, RTW_E_INVALID, "d_rng, d_next, d_weight, d_emitted or d_event is NULL");
    const size_t esz = elem(c);
    if (rays_bytes < n * 6 * esz || next_bytes < n * 6 * esz) return fail(c, RTW_E_INVALID, "d_rays or d_next is smaller than n x 6 values");
    if (hits_bytes < n * 9 * esz) return fail(c, RTW_E_INVALID, "d_hits is smaller than n x 9 values");
    if (ids_bytes < n * 4 * sizeof(int32_t)) return fail(c, RTW_E_INVALID, "d_ids is smaller than n x 4 int32");
    if (rng_bytes < n * 4 * sizeof(uint64_t)) return fail(c, RTW_E_INVALID, "d_rng is smaller than n x 4 uint64");
    if (weight_bytes < n * 3 * esz || emitted_bytes < n * 3 * esz)
        return fail(c, RTW_E_INVALID, "d_weight or d_emitted is smaller than n x 3 values");
    if (event_bytes < n * sizeof(int32_t)) return fail(c, RTW_E_INVALID, "d_event is smaller than n int32");
    if (d_pdfs && pdfs_bytes < n * 3 * esz) return fail(c, RTW_E_INVALID, "d_pdfs is smaller than n x 3 values");
    if (misaligned(d_rays, 6 * esz) || misaligned(d_hits, 9 * esz) || misaligned(d_ids, 16) || misaligned(d_rng, 32) ||
        misaligned(d_next, 6 * esz) || misaligned(d_weight, 3 * esz) || misaligned(d_emitted, 3 * esz) ||
        misaligned(d_pdfs, 3 * esz) || misaligned(d_event, 4))
        return fail(c, RTW_E_INVALID, "a device buffer is not aligned for its records (rtw.h)");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    const ShadeBufs b{d_rays, d_hits, d_ids, d_rng, d_next, d_weight, d_emitted, d_event, d_pdfs};
    return by_precision(c, [&](auto r) { return shade_device_t<decltype(r)>(c, b, n, s); });
}

int rtw_shade_rays(rtw_ctx* c, const void* rays, const void* hits, const int32_t* ids, uint64_t n, uint64_t* rng,
                   void* next, void* weight, void* emitted, int32_t* event, void* pdfs) {
    if (!c) return RTW_E_INVALID;
    int rc = shade_checks(c, rays, hits, ids, n);
    if (rc) return rc;
    if (n == 0) return RTW_OK;
    if (!rng || !next || !weight || !emitted || !event)
        return fail(c, RTW_E_INVALID, "rng, next, weight, emitted or event is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: rays | hits | rng in the queries' ray buffer, the ids in their id buffer,
    // next | weight | emitted | pdfs | event in their record buffer
    const size_t esz = elem(c);
    const size_t rays_b = n * 6 * esz, hits_b = n * 9 * esz, rng_b = n * 4 * sizeof(uint64_t), ids_b = n * 4 * sizeof(int32_t);
    const size_t v3_b = n * 3 * esz, event_b = n * sizeof(int32_t);
    Parts in, out;
    const size_t at_rays = in.add(rays_b), at_hits = in.add(hits_b), at_rng = in.add(rng_b);
    const size_t at_next = out.add(rays_b), at_weight = out.add(v3_b), at_emitted = out.add(v3_b);
    const size_t at_pdfs = out.add(pdfs ? v3_b : 0), at_event = out.add(event_b);
    rc = ensure(c, &q->d_rays, &q->rays_cap, in.total);
    if (!rc) rc = ensure(c, &q->d_out, &q->out_cap, out.total);
    if (!rc) rc = ensure(c, &q->d_ids, &q->ids_cap, ids_b);
    if (rc) return rc;
    char* bi = static_cast<char*>(q->d_rays);
    char* bo = static_cast<char*>(q->d_out);
    HIP_TRY(c, hipMemcpyAsync(bi + at_rays, rays, rays_b, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(bi + at_hits, hits, hits_b, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(bi + at_rng, rng, rng_b, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(q->d_ids, ids, ids_b, hipMemcpyHostToDevice, c->stream));
    const ShadeBufs b{bi + at_rays, bi + at_hits, static_cast<const int32_t*>(q->d_ids),
                      reinterpret_cast<uint64_t*>(bi + at_rng), bo + at_next, bo + at_weight, bo + at_emitted,
                      reinterpret_cast<int32_t*>(bo + at_event), pdfs ? bo + at_pdfs : nullptr};
    rc = by_precision(c, [&](auto r) { return shade_device_t<decltype(r)>(c, b, n, c->stream); });
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(rng, bi + at_rng, rng_b, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(next, bo + at_next, rays_b, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(weight, bo + at_weight, v3_b, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(emitted, bo + at_emitted, v3_b, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(event, bo + at_event, event_b, hipMemcpyDeviceToHost, c->stream));
    if (pdfs) HIP_TRY(c, hipMemcpyAsync(pdfs, bo + at_pdfs, v3_b, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
