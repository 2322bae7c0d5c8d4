// capi_adaptive.cpp -- adaptive sampling (rtw_render_adaptive,
// rtw_render_adaptive_device and their whole-context forms
// rtw_render_adaptive_image, rtw_render_adaptive_image_device): the passes of
// host/render_adaptive.hpp as adaptive passes of capi_render.cpp's render_pass,
// each followed by the fold with the stop vote and the compaction of the tiles
// that go on.  A pass has a launch half that never waits for the device and a
// finish half that does: one device runs them back to back, the ranks of a
// multi-device context run each pass in lockstep -- every rank's launch, then
// every rank's finish -- on the tiles they own, and rank 0 gathers once at the end.
#include <algorithm>

#include "capi_ctx.hpp"
#include "host/render_adaptive.hpp"

namespace {

// The adaptive state of an image of nt tiles, carved from c->d_adapt: doubles
// first (sums nt * 192, s12 nt * 128), then the words.
struct AdaptiveBuffers {
    double *sums, *s12;
    uint32_t *counts, *flags, *list[2], *meta[2];   // meta: {list length, pixels inside the image}
    uint32_t* own;                                   // the tiles of this rank (a rank of several), ascending
};
int adaptive_buffers(rtw_ctx* c, uint32_t nt, AdaptiveBuffers* b) {
    const size_t doubles = (size_t)nt * 64 * 5, words = (size_t)nt * 5 + 4;
    const int rc = ensure(c, &c->d_adapt, &c->adapt_cap, doubles * sizeof(double) + words * sizeof(uint32_t));
    if (rc) return rc;
    b->sums = reinterpret_cast<double*>(c->d_adapt);
    b->s12 = b->sums + (size_t)nt * 64 * 3;
    b->counts = reinterpret_cast<uint32_t*>(b->sums + doubles);
    b->flags = b->counts + nt;
    b->list[0] = b->flags + nt;
    b->list[1] = b->list[0] + nt;
    b->meta[0] = b->list[1] + nt;
    b->meta[1] = b->meta[0] + 2;
    b->own = b->meta[1] + 2;
    return RTW_OK;
}

// the context's two pinned words: the read-back of a pass
int pinned_words(rtw_ctx* c) {
    if (c->h_adapt) return RTW_OK;
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_adapt), 2 * sizeof(uint32_t), hipHostMallocDefault));
    return RTW_OK;
}

// the arguments of a render, shared by its ranks
struct AdaptiveArgs {
    const rtw_camera* cam;
    uint64_t seed;
    uint32_t min_samples, max_samples, window;
    double tolerance;
};

// One context's adaptive render in flight: the tiles still active (list null:
// every tile of the image) and the samples taken so far.
struct AdaptiveRun {
    rtw_ctx* c = nullptr;
    hipStream_t stream = nullptr;
    AdaptiveBuffers b{};
    uint32_t nt = 0;                 // tiles of the image
    uint32_t n_active = 0, first = 0;
    uint64_t active_px = 0, total = 0;
    const uint32_t* list = nullptr;
    int cur = 0;
    bool in_flight = false;          // work queued that finish (or a drain) has not waited for
    bool read_back = false;          // ... ending in the read-back of b.meta[cur]
};

// The render starts on c: the state of the whole image (own null: one device
// renders every tile) or of the tiles `own` of a rank of several.  A rank's
// compaction reads the flag of every tile of the image and its fold writes only
// its own, so the flags and counts start from 0 (d_adapt is carved anew per
// image size: the words may be old sums).
int adaptive_begin(AdaptiveRun& r, rtw_ctx* c, const rtw_camera* cam, hipStream_t stream,
                   const std::vector<uint32_t>* own) {
    const uint32_t W = cam->image_width, H = cam->image_height;
    r.c = c;
    r.stream = stream;
    r.nt = (uint32_t)rtw::n_tiles_of(W, H);
    int rc = adaptive_buffers(c, r.nt, &r.b);
    if (rc) return rc;
    rc = pinned_words(c);
    if (rc) return rc;
    r.n_active = r.nt;
    r.active_px = (uint64_t)W * H;
    if (own) {
        r.n_active = (uint32_t)own->size();
        r.active_px = rtw::tile_pixels(W, H, *own);
        r.list = r.b.own;
        r.in_flight = true;
        HIP_TRY(c, hipMemsetAsync(r.b.counts, 0, (size_t)r.nt * 2 * sizeof(uint32_t), stream));   // counts, flags
        // (from pageable memory: `own` is the caller's again when the call returns)
        if (r.n_active)
            HIP_TRY(c, hipMemcpyAsync(r.b.own, own->data(), own->size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                      stream));
    }
    return RTW_OK;
}

// The launch half of pass k, asynchronous on the run's stream: the render kernel
// on the active tiles (sub-passes under the chunk-sum budget), the fold with the
// stop vote, the compaction of the tiles that go on and the read-back of its
// 8-byte result into pinned memory.  The passes run in tile order (no task
// table): the longest-first cache and the split are left as they are.
template <typename R>
int adaptive_launch(AdaptiveRun& r, const AdaptiveArgs& a, uint32_t k) {
    rtw_ctx* c = r.c;
    const uint32_t W = a.cam->image_width, H = a.cam->image_height;
    const uint32_t end = rtw::adaptive_pass_end(a.min_samples, a.max_samples, a.window, k);
    const bool last = end == a.max_samples;
    const uint32_t cap = rtw::adaptive_sub_samples<R>(c->knobs, r.n_active, device_total(c));
    r.in_flight = true;
    for (uint32_t s = r.first; s < end;) {
        const uint32_t n = std::min(cap, end - s);
        const int rc = render_pass(c, a.cam, a.seed, 0, 1, nullptr, r.stream, rtw::adaptive_pass(s, n, r.list, r.n_active));
        if (rc) return rc;
        rtw::AdaptiveFold f{};
        f.partial = c->d_partial;
        f.n_chunks = a.cam->max_depth ? n : 0;   // depth 0: every sample is 0
        f.list = r.list;
        f.n_active = r.n_active;
        f.sums = r.b.sums;
        f.s12 = r.b.s12;
        f.first = s;
        f.W = W;
        f.H = H;
        f.n_end = end;
        f.decide = s + n == end;
        f.last = last;
        f.tolerance = a.tolerance;
        f.counts = r.b.counts;
        f.flags = r.b.flags;
        if (rtw::launch_fold_adaptive(sizeof(R) == 8, f, r.stream))
            return fail(c, RTW_E_DEVICE, std::string("adaptive fold launch failed: ") + hipGetErrorString(hipGetLastError()));
        s += n;
    }
    r.total += r.active_px * (end - r.first);
    r.first = end;
    if (last) {
        r.n_active = 0;
        return RTW_OK;
    }
    r.cur ^= 1;
    if (rtw::launch_compact_tiles(r.b.flags, r.nt, W, H, r.b.list[r.cur], r.b.meta[r.cur], r.stream))
        return fail(c, RTW_E_DEVICE, std::string("tile compaction launch failed: ") + hipGetErrorString(hipGetLastError()));
    HIP_TRY(c, hipMemcpyAsync(c->h_adapt, r.b.meta[r.cur], 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, r.stream));
    r.read_back = true;
    return RTW_OK;
}

// The finish half: wait for the pass, take the tiles that go on -- the next
// pass is planned for that many.
int adaptive_finish(AdaptiveRun& r) {
    if (!r.read_back) return RTW_OK;
    rtw_ctx* c = r.c;
    r.read_back = false;
    HIP_TRY(c, hipStreamSynchronize(r.stream));
    r.in_flight = false;
    if (c->h_adapt[0] > r.n_active) return fail(c, RTW_E_DEVICE, "adaptive: the active tile list grew");
    r.n_active = c->h_adapt[0];
    r.active_px = c->h_adapt[1];
    r.list = r.b.list[r.cur];
    return RTW_OK;
}

// the render's own stats, once its last work is queued
int adaptive_end(AdaptiveRun& r) {
    HIP_TRY(r.c, hipEventRecord(r.c->ev1, r.stream));   // the stats' time covers the last fold too
    r.c->last.samples = r.total;
    r.c->last.chunk = 1;
    return RTW_OK;
}

// rtw_render_adaptive_device, its arguments checked: the two halves of each
// pass back to back -- one stream synchronisation per pass.
template <typename R>
int render_adaptive_t(rtw_ctx* c, const AdaptiveArgs& a, double* d_sums, uint32_t* d_counts, hipStream_t stream) {
    AdaptiveRun r;
    c->adapt_done = false;   // (d_adapt is this render's from here on: rtw_adaptive_moments)
    int rc = adaptive_begin(r, c, a.cam, stream, nullptr);
    const uint32_t n_passes = rtw::adaptive_passes(a.min_samples, a.max_samples, a.window);
    for (uint32_t k = 0; k < n_passes && r.n_active && !rc; ++k) {
        rc = adaptive_launch<R>(r, a, k);
        if (!rc) rc = adaptive_finish(r);
    }
    if (rc) return rc;
    if (rtw::launch_unpack_adaptive(r.b.sums, r.b.counts, a.cam->image_width, a.cam->image_height, d_sums, d_counts,
                                    stream))
        return fail(c, RTW_E_DEVICE, std::string("adaptive unpack launch failed: ") + hipGetErrorString(hipGetLastError()));
    rc = adaptive_end(r);
    if (rc) return rc;
    c->adapt_done = true;
    c->adapt_w = a.cam->image_width;
    c->adapt_h = a.cam->image_height;
    return RTW_OK;
}

// The passes of an n-rank render, in lockstep: rank k owns the tiles the
// context's split gives it (SplitState::local_tiles: what a fixed render
// renders there) for the whole render and compacts its own list; per pass every
// rank that still has tiles launches on its own device and stream, then each
// finishes.  Afterwards each rank packs its tiles' records for the gather (rank
// 0 in place).  No inter-rank traffic here.
template <typename R>
int adaptive_ranks(rtw_ctx* c, const AdaptiveArgs& a, std::vector<AdaptiveRun>& runs, size_t rank_stride,
                   std::vector<const void*>& src, hipStream_t s0) {
    const uint32_t W = a.cam->image_width, H = a.cam->image_height, n = (uint32_t)runs.size();
    std::vector<uint32_t> own;
    for (uint32_t k = 0; k < n; ++k) {
        rtw_ctx* ck = rtw_device_ctx(c, k);
        HIP_TRY(c, hipSetDevice(ck->device));
        if (k) {
            const int rc = ensure(ck, &ck->d_out, &ck->out_cap, rank_stride * sizeof(double));
            if (rc) return fail(c, rc, ck->err);
            src[k] = ck->d_out;
        }
        c->split.local_tiles(W, H, k, n, own);
        ck->no_work = own.empty();   // a rank without tiles takes no part: the stats of no work
        if (own.empty()) continue;
        const int rc = adaptive_begin(runs[k], ck, a.cam, k ? ck->stream : s0, &own);
        if (rc) return k ? fail(c, rc, ck->err) : rc;
    }
    const uint32_t n_passes = rtw::adaptive_passes(a.min_samples, a.max_samples, a.window);
    for (uint32_t p = 0; p < n_passes; ++p) {
        bool any = false;
        for (uint32_t k = 0; k < n; ++k) {
            if (!runs[k].n_active) continue;
            any = true;
            HIP_TRY(c, hipSetDevice(runs[k].c->device));
            const int rc = adaptive_launch<R>(runs[k], a, p);
            if (rc) return k ? fail(c, rc, runs[k].c->err) : rc;
        }
        if (!any) break;
        for (uint32_t k = 0; k < n; ++k) {
            if (!runs[k].read_back) continue;
            HIP_TRY(c, hipSetDevice(runs[k].c->device));
            const int rc = adaptive_finish(runs[k]);
            if (rc) return k ? fail(c, rc, runs[k].c->err) : rc;
        }
    }
    for (uint32_t k = 0; k < n; ++k) {
        AdaptiveRun& r = runs[k];
        if (!r.c) continue;
        HIP_TRY(c, hipSetDevice(r.c->device));
        double* rec = k ? reinterpret_cast<double*>(r.c->d_out) : reinterpret_cast<double*>(c->d_gather);
        const uint32_t n_own = rtw::tiles_for_rank(W, H, k, n);
        r.in_flight = true;
        if (rtw::launch_pack_adaptive(r.b.own, n_own, r.b.sums, r.b.counts, rec, r.stream))
            return fail(c, RTW_E_DEVICE, std::string("adaptive pack launch failed: ") + hipGetErrorString(hipGetLastError()));
        const int rc = adaptive_end(r);
        if (rc) return k ? fail(c, rc, r.c->err) : rc;
    }
    return RTW_OK;
}

// rtw_render_adaptive_image_device on a multi-device context, its arguments
// checked: the ranks' passes, ONE gather of their records to rank 0, the
// assembly into d_sums / d_counts on s0; the event ordering is
// rtw_render_image_device's.
template <typename R>
int render_adaptive_multi_t(rtw_ctx* c, const AdaptiveArgs& a, double* d_sums, uint32_t* d_counts, hipStream_t s0) {
    const uint32_t W = a.cam->image_width, H = a.cam->image_height, n = rtw_device_count(c);
    // equal-size rank buffers of rank 0's tile count (the most), as the fixed render's
    const size_t stride = std::max<size_t>((size_t)rtw::tiles_for_rank(W, H, 0, n) * rtw::kAdaptiveRecord, 1);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure(c, &c->d_gather, &c->gather_cap, (size_t)n * stride * sizeof(double));
    if (rc) return rc;
    // the assembly's map of a dealt split, before anything is queued (an upload waits for the device)
    const uint32_t* slot = nullptr;
    if (c->split.active(W, H, n)) {
        rc = ensure_tile_slot(c, n);
        if (rc) return rc;
        slot = reinterpret_cast<const uint32_t*>(c->split.d_tile_slot);
    }
    // (the previous call's gather + assembly may still read d_gather on another stream)
    if (c->gather_pending) HIP_TRY(c, hipStreamWaitEvent(s0, c->gather_ev, 0));
    std::vector<AdaptiveRun> runs(n);
    std::vector<const void*> src(n, c->d_gather);
    rc = adaptive_ranks<R>(c, a, runs, stride, src, s0);
    if (!rc) rc = gather_ranks(c, src, stride * sizeof(double), 1, s0);
    if (rc) {
        // the first error is the call's; no buffer stays in use behind it
        for (AdaptiveRun& r : runs)
            if (r.c && r.in_flight && hipSetDevice(r.c->device) == hipSuccess) (void)hipStreamSynchronize(r.stream);
        (void)hipSetDevice(c->device);
        return rc;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (rtw::launch_assemble_adaptive(reinterpret_cast<const double*>(c->d_gather), stride, n, W, H, slot, d_sums,
                                      d_counts, s0))
        return fail(c, RTW_E_DEVICE, std::string("adaptive assembly launch failed: ") + hipGetErrorString(hipGetLastError()));
    rc = gather_done(c, s0);
    if (rc) return rc;
    c->stats_ranks = n;
    return RTW_OK;
}

// what every form refuses before anything else (buffers: the form's own pointers are
// given; multi: the form serves a multi-device context)
int check_adaptive(rtw_ctx* c, const rtw_camera* cam, bool buffers, bool multi, uint32_t min_samples,
                   uint32_t max_samples, uint32_t window, double tolerance) {
    if (!c || !cam || !buffers) return fail(c, RTW_E_INVALID, "bad argument");
    if (c->multi && !multi) return fail(c, RTW_E_UNSUPPORTED, "adaptive sampling of a multi-device context");
    if (!c->has_scene) return fail(c, RTW_E_NO_SCENE, "rtw_set_scene was not called");
    if (const char* why = rtw::adaptive_check(min_samples, max_samples, window, tolerance, c->knobs.chunk))
        return fail(c, RTW_E_INVALID, why);
    return check_image_size(c, cam);
}

// the device forms, `multi` as check_adaptive's
int adaptive_device(rtw_ctx* c, bool multi, const AdaptiveArgs& a, double* d_sums, size_t sums_bytes,
                    uint32_t* d_counts, size_t counts_bytes, void* stream) {
    if (const int rc = check_adaptive(c, a.cam, true, multi, a.min_samples, a.max_samples, a.window, a.tolerance))
        return rc;
    const size_t px = (size_t)a.cam->image_width * a.cam->image_height;
    if (px == 0) return RTW_OK;
    if (!d_sums || !d_counts) return fail(c, RTW_E_INVALID, "d_sums or d_counts is NULL");
    if (sums_bytes < px * 3 * sizeof(double) || counts_bytes < px * sizeof(uint32_t))
        return fail(c, RTW_E_INVALID, "d_sums is smaller than H*W*3 doubles or d_counts than H*W");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = resolve_stream(c, stream);
    if (c->multi)
        return by_precision(c, [&](auto r) { return render_adaptive_multi_t<decltype(r)>(c, a, d_sums, d_counts, s); });
    c->stats_ranks = 1;
    return by_precision(c, [&](auto r) { return render_adaptive_t<decltype(r)>(c, a, d_sums, d_counts, s); });
}

// the host forms
int adaptive_host(rtw_ctx* c, bool multi, const AdaptiveArgs& a, double* sums, uint32_t* counts, rtw_stats* stats) {
    if (const int rc = check_adaptive(c, a.cam, sums && counts, multi, a.min_samples, a.max_samples, a.window,
                                      a.tolerance))
        return rc;
    const size_t px = (size_t)a.cam->image_width * a.cam->image_height;
    if (px == 0) {   // nothing to render: the stats of no samples
        if (stats) {
            *stats = rtw_stats{};
            stats->chunk = 1;
        }
        return RTW_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // the image-order sums, then the counts
    int rc = ensure(c, &c->d_adapt_img, &c->adapt_img_cap, px * (3 * sizeof(double) + sizeof(uint32_t)));
    if (rc) return rc;
    double* d_sums = reinterpret_cast<double*>(c->d_adapt_img);
    uint32_t* d_counts = reinterpret_cast<uint32_t*>(d_sums + px * 3);
    rc = adaptive_device(c, multi, a, d_sums, px * 3 * sizeof(double), d_counts, px * sizeof(uint32_t), nullptr);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(sums, d_sums, px * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(counts, d_counts, px * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return fetch_stats(c, stats);
}

}  // namespace

extern "C" {

int rtw_render_adaptive_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples,
                               uint32_t max_samples, uint32_t window, double tolerance, double* d_sums,
                               size_t sums_bytes, uint32_t* d_counts, size_t counts_bytes, void* stream) {
    return adaptive_device(c, false, AdaptiveArgs{cam, seed, min_samples, max_samples, window, tolerance}, d_sums,
                           sums_bytes, d_counts, counts_bytes, stream);
}

int rtw_render_adaptive(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples, uint32_t max_samples,
                        uint32_t window, double tolerance, double* sums, uint32_t* counts, rtw_stats* stats) {
    return adaptive_host(c, false, AdaptiveArgs{cam, seed, min_samples, max_samples, window, tolerance}, sums, counts,
                         stats);
}

int rtw_render_adaptive_image_device(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples,
                                     uint32_t max_samples, uint32_t window, double tolerance, double* d_sums,
                                     size_t sums_bytes, uint32_t* d_counts, size_t counts_bytes, void* stream) {
    return adaptive_device(c, true, AdaptiveArgs{cam, seed, min_samples, max_samples, window, tolerance}, d_sums,
                           sums_bytes, d_counts, counts_bytes, stream);
}

int rtw_render_adaptive_image(rtw_ctx* c, const rtw_camera* cam, uint64_t seed, uint32_t min_samples,
                              uint32_t max_samples, uint32_t window, double tolerance, double* sums, uint32_t* counts,
                              rtw_stats* stats) {
    return adaptive_host(c, true, AdaptiveArgs{cam, seed, min_samples, max_samples, window, tolerance}, sums, counts,
                         stats);
}

}  // extern "C"
