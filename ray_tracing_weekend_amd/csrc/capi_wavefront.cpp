// capi_wavefront.cpp -- the wavefront path rounds of the C-ABI (include/rtw.h):
// rtw_path_begin_device, rtw_path_advance / rtw_path_advance_device and the
// driver rtw_render_wavefront / rtw_render_wavefront_device.  The driver is
// plan (host/wavefront_plan.hpp) -> per batch: camera rays, begin, rounds of
// closest hit, bounce (the queries' own device forms) and advance, one pinned
// 8-byte readback a round -> fold; on the query state's buffers and events.
#include <algorithm>
#include <string>

#include "capi_ctx.hpp"
#include "host/wavefront_plan.hpp"
#include "wavefront_kernels.h"

namespace {

size_t elem(const rtw_ctx* c) { return c->precision == RTW_F32 ? sizeof(float) : sizeof(double); }

int one_device(rtw_ctx* c) {
    if (c->multi || c->virt || !c->peers.empty())
        return fail(c, RTW_E_UNSUPPORTED, "ray queries run on a one-device context (a query has no tiles to split)");
    return RTW_OK;
}

// the stream argument that resolve_stream turns back into `s`
void* stream_arg(const rtw_ctx* c, hipStream_t s) {
    if (s == c->stream) return nullptr;
    return s ? reinterpret_cast<void*>(s) : RTW_STREAM_NULL;
}

// the query state with the wavefront words: [0] the survivor count, [1 ..] a driver call's totals
int wavefront_state(rtw_ctx* c) {
    int rc = query_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    if (!q->d_wf_words)
        HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&q->d_wf_words), (1 + rtw::kQueryCounters) * sizeof(unsigned long long)));
    if (!q->h_wf_count) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&q->h_wf_count), sizeof(unsigned long long)));
    if (!q->ev_span) HIP_TRY(c, hipEventCreate(&q->ev_span));
    return RTW_OK;
}

struct AdvanceBufs {
    const void* mult;
    const void* res;
    const uint32_t* slot;
    const int32_t* event;
    const void* weight;
    const void* emitted;
    const void* next;
    const uint64_t* rng;
    void* out_rays;
    uint64_t* out_rng;
    void* out_mult;
    void* out_res;
    uint32_t* out_slot;
    void* colour;
    uint64_t colour_slots;
    unsigned long long* count;
};

// zero the count, launch one advance: counters += {rays: n, hits: survivors or SCATTER events}
template <typename R>
int advance_launch_t(rtw_ctx* c, const AdvanceBufs& b, uint64_t n, const double bg[3], bool last,
                     unsigned long long* counters, bool count_scatter, hipStream_t stream) {
    rtw::PathAdvance<R> p{};
    p.event = b.event;
    p.weight = reinterpret_cast<const R*>(b.weight);
    p.emitted = reinterpret_cast<const R*>(b.emitted);
    p.next = reinterpret_cast<const R*>(b.next);
    p.rng = b.rng;
    p.mult = reinterpret_cast<const R*>(b.mult);
    p.res = reinterpret_cast<const R*>(b.res);
    p.slot = b.slot;
    p.out_rays = reinterpret_cast<R*>(b.out_rays);
    p.out_rng = b.out_rng;
    p.out_mult = reinterpret_cast<R*>(b.out_mult);
    p.out_res = reinterpret_cast<R*>(b.out_res);
    p.out_slot = b.out_slot;
    p.colour = reinterpret_cast<R*>(b.colour);
    p.colour_slots = b.colour_slots;
    p.count = b.count;
    p.counters = counters;
    p.n = n;
    for (int q = 0; q < 3; ++q) p.bg[q] = (R)bg[q];
    p.last = last ? 1u : 0u;
    p.count_scatter = count_scatter ? 1u : 0u;
    HIP_TRY(c, hipMemsetAsync(b.count, 0, sizeof(unsigned long long), stream));
    if (n == 0) return RTW_OK;
    if (rtw::launch_path_advance(p, c->knobs.query_grid, stream))
        return fail(c, RTW_E_DEVICE, std::string("path advance launch failed: ") + hipGetErrorString(hipGetLastError()));
    return RTW_OK;
}

// one advance as a query of its own: the query state's counters, events and stats
int advance_query(rtw_ctx* c, const AdvanceBufs& b, uint64_t n, const double bg[3], bool last, hipStream_t stream) {
    QueryState* q = c->query;
    HIP_TRY(c, hipMemsetAsync(q->d_counters, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev0, stream));
    int rc = by_precision(c, [&](auto r) {
        return advance_launch_t<decltype(r)>(c, b, n, bg, last, q->d_counters, false, stream);
    });
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.is_light_pdf = rtw::kQueryPathAdvance;
    q->any = true;
    return RTW_OK;
}

// the host forms' staging: one allocation of 16-byte aligned parts
struct Parts {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t at = total;
        total += align_up(bytes, 16);
        return at;
    }
};

// what the driver refuses before any device call: rtw_shade_rays' refusals and its own
int driver_checks(rtw_ctx* c, const rtw_camera* cam, uint32_t first_sample, uint32_t n_samples, const void* sums,
                  uint32_t batch, rtw::WavefrontPlan& pl) {
    int rc = one_device(c);
    if (rc) return rc;
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (!cam || !sums) return fail(c, RTW_E_INVALID, "cam or sums is NULL");
    if ((uint64_t)first_sample + n_samples > (uint64_t)1 << 32)
        return fail(c, RTW_E_INVALID, "first_sample + n_samples is beyond 2^32");
    const uint32_t n_list = c->precision == RTW_F32 ? c->sc32.n_list : c->sc64.n_list;
    if (n_list == 0 && c->has_lambertian)
        return fail(c, RTW_E_NO_LIGHTS, "rtw_render_wavefront: the light list is empty and the scene holds a Lambertian "
                                        "material (the reference panics, hittable_list.rs:417)");
    pl = rtw::plan_wavefront(cam->image_width, cam->image_height, n_samples, batch, elem(c));
    if (pl.err) return fail(c, pl.err, pl.err_text);
    return RTW_OK;
}

// the driver on device sums [H * W * 3] f64
int driver_run(rtw_ctx* c, const rtw_camera& cam, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
               const rtw::WavefrontPlan& pl, double* d_sums, hipStream_t stream) {
    int rc = wavefront_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    const size_t esz = elem(c);
    const rtw::PathRecords rec = rtw::path_records(esz);
    // the state: two path states, the round's arrays, the colours
    Parts parts;
    size_t at_rays[2], at_rng[2], at_mult[2], at_res[2], at_slot[2];
    for (int k = 0; k < 2; ++k) {
        at_rays[k] = parts.add(pl.rays_bytes), at_rng[k] = parts.add(pl.rng_bytes);
        at_mult[k] = parts.add(pl.vec3_bytes), at_res[k] = parts.add(pl.vec3_bytes), at_slot[k] = parts.add(pl.slot_bytes);
    }
    const size_t at_hits = parts.add(pl.hits_bytes), at_ids = parts.add(pl.ids_bytes), at_next = parts.add(pl.rays_bytes);
    const size_t at_weight = parts.add(pl.vec3_bytes), at_emitted = parts.add(pl.vec3_bytes);
    const size_t at_event = parts.add(pl.event_bytes), at_colour = parts.add(pl.colour_bytes);
    rc = ensure(c, &q->d_wf, &q->wf_cap, parts.total);
    if (rc) return rc;
    char* base = static_cast<char*>(q->d_wf);
    unsigned long long* d_count = q->d_wf_words;
    unsigned long long* d_totals = q->d_wf_words + 1;
    void* sarg = stream_arg(c, stream);
    const uint64_t px = pl.pixels;
    HIP_TRY(c, hipMemsetAsync(d_totals, 0, rtw::kQueryCounters * sizeof(unsigned long long), stream));
    HIP_TRY(c, hipEventRecord(q->ev_span, stream));
    for (uint32_t done = 0; done < n_samples;) {
        const uint32_t B = std::min<uint32_t>(pl.batch, n_samples - done);
        const uint64_t paths = (uint64_t)B * px;
        for (uint32_t b = 0; b < B; ++b) {   // sample done + b: slots [b * px, (b + 1) * px)
            rc = rtw_camera_rays_device(c, &cam, seed, first_sample + done + b, nullptr, 0, 0, px,
                                        base + at_rays[0] + (size_t)b * px * rec.rays, (size_t)px * rec.rays,
                                        reinterpret_cast<uint64_t*>(base + at_rng[0] + (size_t)b * px * rec.rng),
                                        (size_t)px * rec.rng, sarg);
            if (rc) return rc;
        }
        rc = by_precision(c, [&](auto r) {
            using R = decltype(r);
            rtw::PathBegin<R> p{reinterpret_cast<R*>(base + at_mult[0]), reinterpret_cast<R*>(base + at_res[0]),
                                reinterpret_cast<uint32_t*>(base + at_slot[0]), paths, 0u};
            return rtw::launch_path_begin(p, c->knobs.query_grid, stream);
        });
        if (rc) return fail(c, RTW_E_DEVICE, std::string("path begin launch failed: ") + hipGetErrorString(hipGetLastError()));
        // max_depth 0: every path is "alive after max_depth rounds" with res = 0 (camera.rs:470-472)
        if (cam.max_depth == 0) HIP_TRY(c, hipMemsetAsync(base + at_colour, 0, (size_t)paths * rec.vec3, stream));
        uint64_t n = paths;
        int cur = 0;
        for (uint32_t depth = 0; depth < cam.max_depth && n; ++depth) {
            const size_t nn = (size_t)n;
            rc = rtw_hit_rays_device(c, base + at_rays[cur], n, 2.220446049250313e-16 /* f64::EPSILON */, base + at_hits,
                                     nn * rec.hits, reinterpret_cast<int32_t*>(base + at_ids), nn * rec.ids, sarg);
            if (rc) return rc;
            uint64_t* rng = reinterpret_cast<uint64_t*>(base + at_rng[cur]);
            int32_t* event = reinterpret_cast<int32_t*>(base + at_event);
            rc = rtw_shade_rays_device(c, base + at_rays[cur], nn * rec.rays, base + at_hits, nn * rec.hits,
                                       reinterpret_cast<const int32_t*>(base + at_ids), nn * rec.ids, n, rng,
                                       nn * rec.rng, base + at_next, nn * rec.rays, base + at_weight, nn * rec.vec3,
                                       base + at_emitted, nn * rec.vec3, event, nn * rec.event, nullptr, 0, sarg);
            if (rc) return rc;
            const int nxt = cur ^ 1;
            const AdvanceBufs b{base + at_mult[cur], base + at_res[cur], reinterpret_cast<const uint32_t*>(base + at_slot[cur]),
                                event, base + at_weight, base + at_emitted, base + at_next, rng,
                                base + at_rays[nxt], reinterpret_cast<uint64_t*>(base + at_rng[nxt]), base + at_mult[nxt],
                                base + at_res[nxt], reinterpret_cast<uint32_t*>(base + at_slot[nxt]),
                                base + at_colour, paths, d_count};
            rc = by_precision(c, [&](auto r) {
                return advance_launch_t<decltype(r)>(c, b, n, cam.background, depth + 1 == cam.max_depth, d_totals, true,
                                                     stream);
            });
            if (rc) return rc;
            // the round's one readback: the next round's n
            HIP_TRY(c, hipMemcpyAsync(q->h_wf_count, d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            HIP_TRY(c, hipStreamSynchronize(stream));
            n = *q->h_wf_count;
            if (n > paths) return fail(c, RTW_E_DEVICE, "the survivor count is beyond the batch's paths");
            cur = nxt;
        }
        rtw::PathFold f{base + at_colour, d_sums, px * 3, B};
        if (rtw::launch_path_fold(esz == 8, f, c->knobs.query_grid, stream))
            return fail(c, RTW_E_DEVICE, std::string("path fold launch failed: ") + hipGetErrorString(hipGetLastError()));
        done += B;
    }
    // the call's stats: the rounds' totals as the query counters, from ev_span to here
    HIP_TRY(c, hipMemcpyAsync(q->d_counters, d_totals, rtw::kQueryCounters * sizeof(unsigned long long),
                              hipMemcpyDeviceToDevice, stream));
    HIP_TRY(c, hipEventRecord(q->ev1, stream));
    q->last = rtw_query_stats{};
    q->last.is_light_pdf = rtw::kQueryWavefront;
    q->any = true;
    return RTW_OK;
}

rtw::PathArray arr(const void* p, size_t bytes) { return rtw::PathArray{reinterpret_cast<uintptr_t>(p), bytes}; }

}  // namespace

extern "C" {

int rtw_path_begin_device(rtw_ctx* c, uint64_t n, uint32_t first_slot, void* d_mult, size_t mult_bytes, void* d_res,
                          size_t res_bytes, uint32_t* d_slot, size_t slot_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = one_device(c);
    if (rc) return rc;
    if ((uint64_t)first_slot + n > rtw::kWavefrontMaxSlots)
        return fail(c, RTW_E_INVALID, "first_slot + n is beyond 2^32 slots: a slot is a uint32");
    if (n == 0) return RTW_OK;
    if (!d_mult || !d_res || !d_slot) return fail(c, RTW_E_INVALID, "d_mult, d_res or d_slot is NULL");
    const rtw::PathRecords rec = rtw::path_records(elem(c));
    if (mult_bytes < n * rec.vec3 || res_bytes < n * rec.vec3) return fail(c, RTW_E_INVALID, "d_mult or d_res is smaller than n x 3 values");
    if (slot_bytes < n * rec.slot) return fail(c, RTW_E_INVALID, "d_slot is smaller than n uint32");
    const uintptr_t va = rtw::record_align(rec.vec3);
    if (reinterpret_cast<uintptr_t>(d_mult) % va || reinterpret_cast<uintptr_t>(d_res) % va ||
        reinterpret_cast<uintptr_t>(d_slot) % 4)
        return fail(c, RTW_E_INVALID, "a device buffer is not aligned for its records (rtw.h)");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    rc = by_precision(c, [&](auto r) {
        using R = decltype(r);
        rtw::PathBegin<R> p{reinterpret_cast<R*>(d_mult), reinterpret_cast<R*>(d_res), d_slot, n, first_slot};
        return rtw::launch_path_begin(p, c->knobs.query_grid, s);
    });
    if (rc) return fail(c, RTW_E_DEVICE, std::string("path begin launch failed: ") + hipGetErrorString(hipGetLastError()));
    return RTW_OK;
}

int rtw_path_advance_device(rtw_ctx* c, uint64_t n, const void* d_mult, size_t mult_bytes, const void* d_res,
                            size_t res_bytes, const uint32_t* d_slot, size_t slot_bytes, const int32_t* d_event,
                            size_t event_bytes, const void* d_weight, size_t weight_bytes, const void* d_emitted,
                            size_t emitted_bytes, const void* d_next, size_t next_bytes, const uint64_t* d_rng,
                            size_t rng_bytes, void* d_out_rays, size_t out_rays_bytes, uint64_t* d_out_rng,
                            size_t out_rng_bytes, void* d_out_mult, size_t out_mult_bytes, void* d_out_res,
                            size_t out_res_bytes, uint32_t* d_out_slot, size_t out_slot_bytes, void* d_colour,
                            size_t colour_bytes, uint64_t colour_slots, const double background[3], int last,
                            uint64_t* d_count, void* stream) {
    if (!c) return RTW_E_INVALID;
    int rc = one_device(c);
    if (rc) return rc;
    if (!background || !d_count) return fail(c, RTW_E_INVALID, "background or d_count is NULL");
    if (reinterpret_cast<uintptr_t>(d_count) % 8) return fail(c, RTW_E_INVALID, "d_count is not 8-byte aligned");
    const rtw::PathArray in[3] = {arr(d_mult, mult_bytes), arr(d_res, res_bytes), arr(d_slot, slot_bytes)};
    const rtw::PathArray round[5] = {arr(d_event, event_bytes), arr(d_weight, weight_bytes), arr(d_emitted, emitted_bytes),
                                     arr(d_next, next_bytes), arr(d_rng, rng_bytes)};
    const rtw::PathArray out[5] = {arr(d_out_rays, out_rays_bytes), arr(d_out_rng, out_rng_bytes),
                                   arr(d_out_mult, out_mult_bytes), arr(d_out_res, out_res_bytes),
                                   arr(d_out_slot, out_slot_bytes)};
    const char* wrong = rtw::advance_check_arrays(n, elem(c), in, round, out, arr(d_colour, colour_bytes), colour_slots, true);
    if (*wrong) return fail(c, RTW_E_INVALID, std::string("rtw_path_advance_device: ") + wrong);
    HIP_TRY(c, hipSetDevice(c->device));
    rc = query_state(c);
    if (rc) return rc;
    hipStream_t s = resolve_stream(c, stream);
    const AdvanceBufs b{d_mult, d_res, d_slot, d_event, d_weight, d_emitted, d_next, d_rng, d_out_rays, d_out_rng,
                        d_out_mult, d_out_res, d_out_slot, d_colour, colour_slots,
                        reinterpret_cast<unsigned long long*>(d_count)};
    return advance_query(c, b, n, background, last != 0, s);
}

int rtw_path_advance(rtw_ctx* c, uint64_t n, const void* mult, const void* res, const uint32_t* slot,
                     const int32_t* event, const void* weight, const void* emitted, const void* next,
                     const uint64_t* rng, void* out_rays, uint64_t* out_rng, void* out_mult, void* out_res,
                     uint32_t* out_slot, void* colour, uint64_t colour_slots, const double background[3], int last,
                     uint64_t* survivors) {
    if (!c) return RTW_E_INVALID;
    int rc = one_device(c);
    if (rc) return rc;
    if (!background || !survivors) return fail(c, RTW_E_INVALID, "background or survivors is NULL");
    const rtw::PathArray in[3] = {arr(mult, 0), arr(res, 0), arr(slot, 0)};
    const rtw::PathArray round[5] = {arr(event, 0), arr(weight, 0), arr(emitted, 0), arr(next, 0), arr(rng, 0)};
    const rtw::PathArray out[5] = {arr(out_rays, 0), arr(out_rng, 0), arr(out_mult, 0), arr(out_res, 0), arr(out_slot, 0)};
    const char* wrong = rtw::advance_check_arrays(n, elem(c), in, round, out, arr(colour, 0), colour_slots, false);
    if (*wrong) return fail(c, RTW_E_INVALID, std::string("rtw_path_advance: ") + wrong);
    *survivors = 0;
    if (n == 0) return RTW_OK;
    // a slot beyond the colour array is the caller's error: the host form reads every one
    for (uint64_t k = 0; k < n; ++k)
        if (slot[k] >= colour_slots) return fail(c, RTW_E_INVALID, "rtw_path_advance: a slot is beyond colour_slots");
    HIP_TRY(c, hipSetDevice(c->device));
    rc = wavefront_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    // staging: the in-state and the round in the queries' ray buffer, the out-state and
    // the colours in their record buffer
    const rtw::PathRecords rec = rtw::path_records(elem(c));
    const size_t nn = (size_t)n, v3_b = nn * rec.vec3, rays_b = nn * rec.rays, rng_b = nn * rec.rng;
    const size_t slot_b = nn * rec.slot, event_b = nn * rec.event, colour_b = (size_t)colour_slots * rec.vec3;
    Parts pi, po;
    const size_t i_mult = pi.add(v3_b), i_res = pi.add(v3_b), i_slot = pi.add(slot_b), i_event = pi.add(event_b);
    const size_t i_weight = pi.add(v3_b), i_emitted = pi.add(v3_b), i_next = pi.add(rays_b), i_rng = pi.add(rng_b);
    const size_t o_rays = po.add(rays_b), o_rng = po.add(rng_b), o_mult = po.add(v3_b), o_res = po.add(v3_b);
    const size_t o_slot = po.add(slot_b), o_colour = po.add(colour_b);
    rc = ensure(c, &q->d_rays, &q->rays_cap, pi.total);
    if (!rc) rc = ensure(c, &q->d_out, &q->out_cap, po.total);
    if (rc) return rc;
    char* bi = static_cast<char*>(q->d_rays);
    char* bo = static_cast<char*>(q->d_out);
    hipStream_t s = c->stream;
    const struct {
        size_t at;
        const void* from;
        size_t bytes;
    } up[8] = {{i_mult, mult, v3_b},       {i_res, res, v3_b},         {i_slot, slot, slot_b}, {i_event, event, event_b},
               {i_weight, weight, v3_b},   {i_emitted, emitted, v3_b}, {i_next, next, rays_b}, {i_rng, rng, rng_b}};
    for (const auto& u : up) HIP_TRY(c, hipMemcpyAsync(bi + u.at, u.from, u.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(bo + o_colour, colour, colour_b, hipMemcpyHostToDevice, s));
    const AdvanceBufs b{bi + i_mult, bi + i_res, reinterpret_cast<const uint32_t*>(bi + i_slot),
                        reinterpret_cast<const int32_t*>(bi + i_event), bi + i_weight, bi + i_emitted, bi + i_next,
                        reinterpret_cast<const uint64_t*>(bi + i_rng), bo + o_rays, reinterpret_cast<uint64_t*>(bo + o_rng),
                        bo + o_mult, bo + o_res, reinterpret_cast<uint32_t*>(bo + o_slot), bo + o_colour, colour_slots,
                        q->d_wf_words};
    rc = advance_query(c, b, n, background, last != 0, s);
    if (rc) {
        (void)hipStreamSynchronize(s);   // (the uploads read the caller's arrays)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(q->h_wf_count, q->d_wf_words, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(colour, bo + o_colour, colour_b, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    const uint64_t m = *q->h_wf_count;
    if (m > n) return fail(c, RTW_E_DEVICE, "the survivor count is beyond n");
    const size_t mm = (size_t)m;
    if (m) {   // the survivors' rows; the rest of the out-state is left as it was
        HIP_TRY(c, hipMemcpyAsync(out_rays, bo + o_rays, mm * rec.rays, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(out_rng, bo + o_rng, mm * rec.rng, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(out_mult, bo + o_mult, mm * rec.vec3, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(out_res, bo + o_res, mm * rec.vec3, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipMemcpyAsync(out_slot, bo + o_slot, mm * rec.slot, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    *survivors = m;
    return RTW_OK;
}

int rtw_render_wavefront_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample,
                                uint32_t n_samples, uint32_t batch, double* d_sums, size_t sums_bytes, void* stream) {
    if (!c) return RTW_E_INVALID;
    rtw::WavefrontPlan pl;
    int rc = driver_checks(c, cam, first_sample, n_samples, d_sums, batch, pl);
    if (rc) return rc;
    if (sums_bytes < pl.sums_bytes) return fail(c, RTW_E_INVALID, "d_sums is smaller than H x W x 3 doubles");
    if (reinterpret_cast<uintptr_t>(d_sums) % 8) return fail(c, RTW_E_INVALID, "d_sums is not 8-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    return driver_run(c, *cam, seed, first_sample, n_samples, pl, d_sums, resolve_stream(c, stream));
}

int rtw_render_wavefront(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
                         uint32_t batch, double* sums) {
    if (!c) return RTW_E_INVALID;
    rtw::WavefrontPlan pl;
    int rc = driver_checks(c, cam, first_sample, n_samples, sums, batch, pl);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    rc = wavefront_state(c);
    if (rc) return rc;
    QueryState* q = c->query;
    rc = ensure(c, &q->d_wf_sums, &q->wf_sums_cap, pl.sums_bytes);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(q->d_wf_sums, sums, pl.sums_bytes, hipMemcpyHostToDevice, c->stream));
    rc = driver_run(c, *cam, seed, first_sample, n_samples, pl, static_cast<double*>(q->d_wf_sums), c->stream);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);   // (the upload reads `sums`)
        return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(sums, q->d_wf_sums, pl.sums_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTW_OK;
}

}  // extern "C"
